"""Host replica of ``sal.refit_exposures``, vectorised over the problems with a latch mask.

A problem is one row x of a count matrix against fixed signatures W (K, V), rows of sum one:
    x = max(x, EPSILON);  h_k = sum(x) / K
    step:       wh = h W;  a = x / wh;  h_k <- max(h_k sum_v W[k, v] a_v, EPSILON)
    objective:  sum_v x log(x / wh) - x + wh   (the sample's KL divergence on the clipped x), at iteration 0 and at every
                multiple of conv_test_freq
    stop:       first test at or after min_iterations with |prev - cur| / |prev| < tol (NaN: false), converged; otherwise
                at max_iterations.  A stopped problem's h is latched.
``dtype`` is float64 or ``np.longdouble``; ``perm`` permutes the features (another summation order over v, same
mathematics); ``schedule`` forces each problem's stop iteration instead of testing; ``free_run`` latches nothing and
records every test's relative change for every problem.
"""

from types import SimpleNamespace

import numpy as np

EPSILON = float(np.finfo(np.float32).eps)


def normalize(S):
    S = np.asarray(S, dtype=np.float64)
    return S / S.sum(axis=1, keepdims=True)


def start(x, K):
    return np.repeat(x.sum(axis=1, keepdims=True) / K, K, axis=1)


def _wh(h, W):
    # (einsum's own loops, not BLAS: a row's sums do not depend on how many rows there are)
    return np.einsum("pk,kv->pv", h, W)


def step(x, W, h):
    a = x / _wh(h, W)
    return np.maximum(h * np.einsum("pv,kv->pk", a, W), h.dtype.type(EPSILON))


def objective(x, W, h):
    wh = _wh(h, W)
    return (x * np.log(x / wh) - x + wh).sum(axis=1)


def quantile_indices(quantiles, R):
    q = np.asarray(quantiles, dtype=np.float64).reshape(-1)
    pos = q * float(R - 1)
    return np.clip(np.where(q <= 0.5, np.floor(pos), np.ceil(pos)), 0, R - 1).astype(np.int64)


def reduce_resamples(Hr, quantiles):
    """(mean, quantiles) of exposures_resampled (R, N, K) by the stated rules: sum in ascending r / R; order statistics."""
    R = Hr.shape[0]
    total = np.zeros(Hr.shape[1:], dtype=np.float64)
    for r in range(R):
        total = total + Hr[r]
    srt = np.sort(Hr, axis=0)
    return total / R, srt[quantile_indices(quantiles, R)]


def refit(X, W, min_iterations=500, max_iterations=10000, conv_test_freq=10, tol=1e-7, dtype=np.float64, perm=None, schedule=None,
          free_run=False):
    X = np.asarray(X, dtype=np.float64)
    W = np.asarray(W, dtype=np.float64)
    if perm is not None:
        X, W = X[:, perm], W[:, perm]
    x = np.maximum(X, EPSILON).astype(dtype)
    W = W.astype(dtype)
    P, K = x.shape[0], W.shape[0]
    h = start(x, K)
    stopped = np.zeros(P, dtype=bool)
    nit = np.zeros(P, dtype=np.int64)
    conv = np.zeros(P, dtype=bool)
    err = np.zeros(P, dtype=dtype)
    prev = objective(x, W, h)
    err[:] = prev
    changes, tests = [], []
    last = int(max_iterations if schedule is None else np.max(schedule))
    if schedule is not None:
        schedule = np.asarray(schedule, dtype=np.int64)
        stopped = schedule == 0
    for it in range(1, last + 1):
        if stopped.all():
            break
        h = np.where(stopped[:, None], h, step(x, W, h))
        at_test = it % conv_test_freq == 0
        if schedule is not None:
            now = ~stopped & (schedule == it)
            if now.any():
                cur = objective(x, W, h)
                err[now], nit[now] = cur[now], it
                stopped |= now
            continue
        if not (at_test or it == max_iterations):
            continue
        cur = objective(x, W, h)
        live = ~stopped
        if at_test:
            with np.errstate(invalid="ignore", divide="ignore"):
                rel = np.abs(prev - cur) / np.abs(prev)
            if free_run:
                changes.append(rel.copy())
                tests.append(it)
            elif it >= min_iterations:
                hit = live & (rel < tol)
                conv |= hit
                err[hit], nit[hit] = cur[hit], it
                stopped |= hit
        if it == max_iterations and not free_run:
            end = ~stopped
            err[end], nit[end] = cur[end], it
            stopped |= end
        prev = np.where(live, cur, prev)
    if free_run:
        nit[:] = last
        err = objective(x, W, h)
    return SimpleNamespace(exposures=h, reconstruction_errors=err, n_iterations=nit, converged=conv,
                           changes=np.array(changes).reshape(len(tests), P), tests=np.array(tests, dtype=np.int64))


def poisson_catalogue(N, K, V=96, seed=0, mutations=(200, 20000), zero_heavy=0):
    """(counts (N, V), signatures (K, V)): Dirichlet signatures, sparse exposures, Poisson counts; the last ``zero_heavy``
    rows carry a handful of mutations only."""
    rng = np.random.default_rng(seed)
    S = rng.dirichlet(np.full(V, 0.15), size=K)
    E = rng.dirichlet(np.full(K, 0.3), size=N) * rng.uniform(*mutations, size=(N, 1))
    X = rng.poisson(E @ S).astype(np.float64)
    for i in range(zero_heavy):
        X[N - 1 - i] = 0.0
        X[N - 1 - i, rng.integers(0, V, size=3)] = rng.integers(1, 4, size=3)
    return X, normalize(S)
