"""A NumPy replica of ``sal.profile_likelihood`` and ``sal.exposure_intervals`` (``csrc/salnmf_profile.h``)
-- TESTS ONLY.

Written from the contract.  For sample n with candidate set C, a signature s in C with |C| >= 2, and a value c >= 0:
    the frozen solve starts from h_s = c, h_k = sum(x) / (|C| - 1) on C \\ {s}, 0.0 off C; every step is ``_refit_ref.step``
    applied to the members of C \\ {s} only (an entry that is 0.0 stays 0.0, h_s is never touched); objective and stop rule are
    the refit's, as ``_assign_masks_ref.assign`` applies them: the iteration-0 test, then every conv_test_freq;
    f(c) is the objective it stops at, g(c) = f(c) - f1 with f1 the solve on C (``_presence_ref.solve``).
The search rule is a generator that yields a trial value and is sent g at it, so that it is a pure function of g: ``search``
drives it with a callable, ``replay`` with recorded values, ``intervals`` drives every pair's two ends in lockstep on batched
frozen solves.
"""

from types import SimpleNamespace

import numpy as np

import _presence_ref as presence_ref
import _refit_ref as refit_ref

EPSILON = refit_ref.EPSILON


def frozen_solve(X, W, C, s, c, min_iterations=500, max_iterations=10000, conv_test_freq=10, tol=1e-7):
    """Row p of X on its set C[p] with entry s[p] frozen at c[p] -> exposures, reconstruction_errors, n_iterations, converged.
    Rows are independent (``_refit_ref._wh``), so the rows that have stopped are left out of the later steps."""
    if max_iterations % conv_test_freq:
        raise ValueError("max_iterations must be a multiple of conv_test_freq")
    x = np.maximum(np.asarray(X, dtype=np.float64), EPSILON)
    W = np.asarray(W, dtype=np.float64)
    P, K = x.shape[0], W.shape[0]
    rows = np.arange(P)
    s = np.broadcast_to(np.asarray(s, dtype=np.int64), (P,))
    c = np.broadcast_to(np.asarray(c, dtype=np.float64), (P,))
    free = np.asarray(C, dtype=bool).copy()
    assert free[rows, s].all() and (free.sum(axis=1) >= 2).all()
    free[rows, s] = False
    frozen = np.zeros((P, K), dtype=bool)
    frozen[rows, s] = True
    h = np.where(free, (x.sum(axis=1) / free.sum(axis=1))[:, None], 0.0)
    h[rows, s] = c
    done = np.zeros(P, dtype=bool)
    prev = np.zeros(P)
    f, nit, conv = np.zeros(P), np.zeros(P, dtype=np.int64), np.zeros(P, dtype=bool)
    it = 0
    while True:
        live = np.flatnonzero(~done)
        if it % conv_test_freq == 0:
            cur = refit_ref.objective(x[live], W, h[live])
            with np.errstate(invalid="ignore", divide="ignore"):
                rel = np.abs(prev[live] - cur) / np.abs(prev[live])
            hit = (it > 0) & (it >= min_iterations) & (rel < tol)
            stop = hit | (it == max_iterations)
            prev[live] = cur
            f[live[stop]], nit[live[stop]], conv[live[stop]] = cur[stop], it, hit[stop]
            done[live[stop]] = True
            live = live[~stop]
            if not live.size:
                break
        hl = h[live]
        h[live] = np.where((hl == 0.0) | frozen[live], hl, refit_ref.step(x[live], W, hl))
        it += 1
    return SimpleNamespace(exposures=h, reconstruction_errors=f, n_iterations=nit, converged=conv)


def search_end(upper, estimate, delta, n_bisections, max_expansions):
    """The search of one end as a generator: yields a trial value, is sent g there, returns (end, bracketed).  A comparison with
    a NaN is false."""
    hh = float(estimate)
    if not upper:
        # n_bisections halvings; while the bracket still starts at 0.0 after them, up to max_expansions more, to the first
        # trial outside
        lo, hi, n = 0.0, hh, 0
        while n < n_bisections or (not lo > 0.0 and n < n_bisections + max_expansions):
            m = 0.5 * (lo + hi)
            n += 1
            if (yield m) > delta:
                lo = m
            else:
                hi = m
        return lo, True
    d = hh if hh > 1.0 else 1.0
    lo, hi = hh, None
    for e in range(max_expansions):
        c = hh + d * 2.0**e
        if (yield c) > delta:
            hi = c
            break
        lo = c
    if hi is None:
        return np.inf, False
    for _ in range(n_bisections):
        m = 0.5 * (lo + hi)
        if (yield m) > delta:
            hi = m
        else:
            lo = m
    return hi, True


def drive(rule, g):
    """Runs one end's generator on the callable g -> (end, bracketed, trial values, their g)."""
    values, profile = [], []
    try:
        c = next(rule)
        while True:
            values.append(c)
            profile.append(float(g(c)))
            c = rule.send(profile[-1])
    except StopIteration as stop:
        end, bracketed = stop.value
    return end, bracketed, values, profile


def search(g, estimate, g0, delta=1.92, n_bisections=16, max_expansions=40):
    """Both ends of one pair from a callable g (or one callable per end) -> lower, upper, bracketed, n_trials (2,), trace_values and trace_profile
    (2, max_expansions + n_bisections) NaN past the trials.  ``g0 <= delta`` gives lower 0.0 without a trial."""
    T = max_expansions + n_bisections
    trace_values, trace_profile = np.full((2, T), np.nan), np.full((2, T), np.nan)
    n_trials = np.zeros(2, dtype=np.int32)
    lower, bracketed = 0.0, False
    for which in (0, 1):
        if which == 0 and g0 <= delta:
            continue
        end, br, values, profile = drive(search_end(which == 1, estimate, delta, n_bisections, max_expansions), g if callable(g) else g[which])
        n_trials[which] = len(values)
        trace_values[which, : len(values)], trace_profile[which, : len(values)] = values, profile
        if which == 0:
            lower = end
        else:
            upper, bracketed = end, br
    return SimpleNamespace(lower=lower, upper=upper, bracketed=bracketed, n_trials=n_trials, trace_values=trace_values, trace_profile=trace_profile)


def replay(trace_profile, estimate, g0, **kw):
    """``search`` fed with recorded g values (2, T), each end's in its trial order, instead of solves: what the rule does with
    them."""
    feeds = [iter(np.asarray(row, dtype=np.float64).tolist()) for row in trace_profile]
    return search((lambda c: next(feeds[0]), lambda c: next(feeds[1])), estimate, g0, **kw)


def observed(X, W, test, candidates=None, **kw):
    """(C, tested, exposures (N, K), f1 (N,)): the alternative fit of every sample with a tested pair."""
    X = np.asarray(X, dtype=np.float64)
    N, K = X.shape[0], W.shape[0]
    C = presence_ref.candidate_sets(candidates, N, K)
    tested = presence_ref.tested_pairs(C, test)
    exposures, errors = np.full((N, K), np.nan), np.full(N, np.nan)
    rows = np.flatnonzero(tested.any(axis=1))
    if rows.size:
        alt = presence_ref.solve(X[rows], W, C[rows], **kw)
        exposures[rows], errors[rows] = alt.exposures, alt.reconstruction_errors
    return C, tested, exposures, errors


def profile(counts, signatures, test, values, candidates=None, **kw):
    """``sal.profile_likelihood`` on the host; ``values`` of shape (M,) or (N, S, M)."""
    X = np.asarray(counts, dtype=np.float64)
    W = refit_ref.normalize(signatures)
    N, K, S = X.shape[0], W.shape[0], len(test)
    C, tested, exposures, errors = observed(X, W, test, candidates, **kw)
    values = np.asarray(values, dtype=np.float64)
    M = values.shape[-1]
    grid = np.broadcast_to(values, (N, S, M))
    f, g = np.full((N, S, M), np.nan), np.full((N, S, M), np.nan)
    nit, conv = np.zeros((N, S, M), dtype=np.int64), np.zeros((N, S, M), dtype=bool)
    H = np.full((N, S, M, K), np.nan)
    for j, s in enumerate(test):
        rows = np.flatnonzero(tested[:, j])
        for i in range(M if rows.size else 0):
            res = frozen_solve(X[rows], W, C[rows], s, grid[rows, j, i], **kw)
            f[rows, j, i], nit[rows, j, i], conv[rows, j, i], H[rows, j, i] = res.reconstruction_errors, res.n_iterations, res.converged, res.exposures
            g[rows, j, i] = res.reconstruction_errors - errors[rows]
    return SimpleNamespace(profile=g, errors=f, n_iterations=nit, converged=conv, profile_exposures=H, exposures=exposures, reconstruction_errors=errors,
                           tested=tested, candidates=C)


def intervals(counts, signatures, test, candidates=None, max_kl_increase=1.92, n_bisections=16, max_expansions=40, **kw):
    """``sal.exposure_intervals`` on the host: every end's ``search_end`` generator, advanced in lockstep on batched frozen solves."""
    X = np.asarray(counts, dtype=np.float64)
    W = refit_ref.normalize(signatures)
    N, S, T = X.shape[0], len(test), max_expansions + n_bisections
    C, tested, exposures, errors = observed(X, W, test, candidates, **kw)
    nan = np.nan
    lower, upper, estimate = np.full((N, S), nan), np.full((N, S), nan), np.full((N, S), nan)
    statistic, null_errors = np.full((N, S), nan), np.full((N, S), nan)
    bracketed, n_trials = np.zeros((N, S), dtype=bool), np.zeros((N, S, 2), dtype=np.int32)
    trace_values, trace_profile = np.full((N, S, 2, T), nan), np.full((N, S, 2, T), nan)
    for j, s in enumerate(test):
        rows = np.flatnonzero(tested[:, j])
        if not rows.size:
            continue
        null = frozen_solve(X[rows], W, C[rows], s, 0.0, **kw)
        null_errors[rows, j] = null.reconstruction_errors
        statistic[rows, j] = null.reconstruction_errors - errors[rows]
        estimate[rows, j] = exposures[rows, s]
    # the ends that need trials, each with its generator and its pending trial value
    ends = []
    for n, j in zip(*np.nonzero(tested)):
        lower[n, j] = 0.0
        for which in (0, 1):
            if which == 0 and statistic[n, j] <= max_kl_increase:
                continue
            rule = search_end(which == 1, estimate[n, j], max_kl_increase, n_bisections, max_expansions)
            try:
                ends.append([n, j, which, rule, next(rule)])
            except StopIteration as stop:  # (no trial allowed)
                lower[n, j] = stop.value[0]
    while ends:
        rows = np.array([e[0] for e in ends])
        sig = np.array([test[e[1]] for e in ends])
        res = frozen_solve(X[rows], W, C[rows], sig, np.array([e[4] for e in ends]), **kw)
        g = res.reconstruction_errors - errors[rows]
        still = []
        for e, ge in zip(ends, g):
            n, j, which, rule, c = e
            trace_values[n, j, which, n_trials[n, j, which]], trace_profile[n, j, which, n_trials[n, j, which]] = c, ge
            n_trials[n, j, which] += 1
            try:
                e[4] = rule.send(float(ge))
                still.append(e)
            except StopIteration as stop:
                if which == 0:
                    lower[n, j] = stop.value[0]
                else:
                    upper[n, j], bracketed[n, j] = stop.value
        ends = still
    return SimpleNamespace(lower=lower, upper=upper, estimate=estimate, bracketed=bracketed, n_trials=n_trials, statistic=statistic,
                           null_errors=null_errors, exposures=exposures, reconstruction_errors=errors, tested=tested, candidates=C,
                           trace_values=trace_values, trace_profile=trace_profile)


def coverage_samples(seed=20250, n_samples=200):
    """The samples of the coverage tests, host and device: (counts (200, 96), catalogue (4, 96), true exposures (200, 4)).  Poisson
    counts of about 2000 mutations; signatures 0, 1 and 2 carry shares of at least a tenth each (interior exposures),
    signature 3 is truly absent."""
    rng = np.random.default_rng(seed)
    V, K, total = 96, 4, 2000.0
    S = refit_ref.normalize(rng.dirichlet(np.full(V, 0.15), size=K))
    shares = 0.1 + 0.7 * rng.dirichlet(np.full(K - 1, 1.0), size=n_samples)
    E = np.concatenate([total * shares, np.zeros((n_samples, 1))], axis=1)
    X = rng.poisson(E @ S).astype(np.float64)
    return X, S, E
