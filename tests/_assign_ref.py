"""Host replica of ``sal.assign_signatures``, on the functions of ``tests/_refit_ref.py``.

A problem is a row x = max(row, EPSILON) against W (K, V).  A SOLVE from a start h with an active set A is the refit's
iteration on the active entries (``_refit_ref.step`` / ``objective``, the refit's stop rule, iterations counted from 0 at the
start of the solve, the objective at iteration 0 and every multiple of conv_test_freq); inactive entries are exactly 0.0 and
stay 0.0.  Phase 0: A = all K, h_k = sum(x) / K.  Rounds: candidate c = the active, not yet protected signature of smallest h,
lowest index on equal values; stop when there is none or |A| == 1; trial: h with entry c set to 0.0, solved with A \\ {c}; if
f' - f <= max_kl_increase (false for a NaN) the trial's h, f, A are accepted, otherwise c is protected for good.

The problems advance together, one global iteration at a time, each in its own solve (``_refit_ref``'s sums over a row do
not depend on the other rows, so a problem's numbers are those of a run on its own).  ``trials[p]`` records every decision
with what isolates it: the candidate, its value, the runner-up's value (inf without one), f' - f and the verdict.
"""

from types import SimpleNamespace

import numpy as np

import _refit_ref as ref

EPSILON = ref.EPSILON


def check(max_iterations, conv_test_freq, max_kl_increase):
    if conv_test_freq < 1 or max_iterations % conv_test_freq != 0:
        raise ValueError("max_iterations must be a multiple of conv_test_freq")
    if not np.isfinite(max_kl_increase):
        raise ValueError("max_kl_increase must be finite")


def candidate(h, eligible):
    """(index, value, runner-up value) of the smallest eligible entry, lowest index on equal values; index -1 without one."""
    best, value, runner = -1, np.inf, np.inf
    for k in np.flatnonzero(eligible):
        if h[k] < value:
            best, value, runner = int(k), h[k], value
        elif h[k] < runner:
            runner = h[k]
    return best, value, runner


def assign(X, W, max_kl_increase=1.92, min_iterations=500, max_iterations=10000, conv_test_freq=10, tol=1e-7, dtype=np.float64, perm=None):
    check(max_iterations, conv_test_freq, max_kl_increase)
    X = np.asarray(X, dtype=np.float64)
    W = np.asarray(W, dtype=np.float64)
    if perm is not None:
        X, W = X[:, perm], W[:, perm]
    x = np.maximum(X, EPSILON).astype(dtype)
    W = W.astype(dtype)
    P, K = x.shape[0], W.shape[0]
    h = ref.start(x, K)
    accepted = h.copy()
    active = np.ones((P, K), dtype=bool)
    protected = np.zeros((P, K), dtype=bool)
    mode = np.zeros(P, dtype=np.int64)  # 0: phase 0, 1: a trial, 2: finished
    fresh = np.zeros(P, dtype=bool)
    itl = np.zeros(P, dtype=np.int64)
    cand = np.zeros(P, dtype=np.int64)
    prev = np.zeros(P, dtype=dtype)
    f = np.zeros(P, dtype=dtype)
    n_trials = np.zeros(P, dtype=np.int64)
    n_iterations = np.zeros(P, dtype=np.int64)
    converged = np.ones(P, dtype=bool)
    removal_round = np.full((P, K), -1, dtype=np.int64)
    kl_increase = np.full((P, K), np.nan, dtype=dtype)
    dense = SimpleNamespace(exposures=np.zeros((P, K), dtype=dtype), reconstruction_errors=np.zeros(P, dtype=dtype),
                            n_iterations=np.zeros(P, dtype=np.int64), converged=np.zeros(P, dtype=bool))
    trials = [[] for _ in range(P)]
    g = 0
    while True:
        if g % conv_test_freq == 0:
            repass = False
            while True:
                cur = ref.objective(x, W, h)
                todo = (mode != 2) & (fresh | (not repass))
                with np.errstate(invalid="ignore", divide="ignore"):
                    rel = np.abs(prev - cur) / np.abs(prev)
                hit = todo & (itl > 0) & (itl >= min_iterations) & (rel < tol)
                stop = hit | (todo & (itl == max_iterations))
                prev = np.where(todo, cur, prev)
                fresh[:] = False
                for p in np.flatnonzero(stop):
                    n_iterations[p] += itl[p]
                    converged[p] &= bool(hit[p])
                    if mode[p] == 0:
                        dense.exposures[p], dense.reconstruction_errors[p] = h[p], cur[p]
                        dense.n_iterations[p], dense.converged[p] = itl[p], hit[p]
                        accept = True
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
                    c, value, runner = candidate(h[p], active[p] & ~protected[p])
                    if c < 0 or active[p].sum() == 1:
                        mode[p] = 2
                    else:
                        trials[p].append(dict(candidate=c, value=value, runner=runner))
                        cand[p], mode[p], itl[p], fresh[p] = c, 1, 0, True
                        h[p, c] = 0.0
                if not fresh.any():
                    break
                repass = True
        if (mode == 2).all():
            break
        live = mode != 2
        h = np.where(live[:, None], np.where(h == 0.0, h, ref.step(x, W, h)), h)
        itl[live] += 1
        g += 1
    return SimpleNamespace(exposures=h, active=active, reconstruction_errors=f, removal_round=removal_round, kl_increase=kl_increase,
                           n_trials=n_trials, n_iterations=n_iterations, converged=converged, dense=dense, trials=trials)


def isolation(runs, max_kl_increase, rel=1e-6):
    """Per problem: do the replicas `runs` agree on every choice, does every threshold comparison clear the threshold by
    rel * max(1, |threshold|), and is every chosen candidate either bit-equal to EPSILON or a relative `rel` below the
    runner-up?  Also returns the smallest threshold margin seen, as a fraction of max(1, |threshold|)."""
    P = len(runs[0].trials)
    scale = max(1.0, abs(max_kl_increase))
    ok = np.ones(P, dtype=bool)
    margin = np.inf
    for p in range(P):
        first = runs[0].trials[p]
        for run in runs:
            mine = run.trials[p]
            if [(t["candidate"], t["accepted"]) for t in mine] != [(t["candidate"], t["accepted"]) for t in first]:
                ok[p] = False
            for t in mine:
                m = abs(float(t["delta"]) - max_kl_increase) / scale
                margin = min(margin, m)
                tied_at_floor = float(t["value"]) == EPSILON
                if not (m >= rel) or not (tied_at_floor or float(t["value"]) <= float(t["runner"]) * (1 - rel)):
                    ok[p] = False
    return ok, margin


def planted_catalogue(N=12, K=12, V=96, n_planted=3, seed=5, mutations=(450, 3500)):
    """(counts, signatures, planted support): rows with `n_planted` of K Dirichlet(0.15) signatures, each with at
    least a seventh of the row's mutations."""
    rng = np.random.default_rng(seed)
    S = rng.dirichlet(np.full(V, 0.15), size=K)
    planted = np.zeros((N, K), dtype=bool)
    E = np.zeros((N, K))
    for n in range(N):
        idx = rng.choice(K, size=n_planted, replace=False)
        planted[n, idx] = True
        share = rng.uniform(0.5, 1.5, size=n_planted)
        E[n, idx] = share / share.sum() * rng.uniform(*mutations)
    X = rng.poisson(E @ S).astype(np.float64)
    return X, ref.normalize(S), planted
