"""Host replica of ``sal.nb_refit_exposures`` and ``sal.estimate_dispersion``, vectorised over the
problems with a latch mask, modelled on tests/_refit_ref.py.

A problem is one row x of a count matrix against fixed signatures W (K, V), rows of sum one, with its own dispersion alpha:
    x = max(x, EPSILON);  h_k = sum(x) / K
    step:       p = h W;  a = x / p;  b = (x + alpha) / (p + alpha);  h_k <- max(h_k (sum_v W[k, v] a_v) / (sum_v W[k, v] b_v), EPSILON)
    objective:  sum_v x log(x / p) - (x + alpha) log((x + alpha) / (p + alpha)), at iteration 0 and at every multiple of
                conv_test_freq
    stop:       first test at or after min_iterations with |prev - cur| / |prev| < tol (NaN: false), converged; otherwise
                at max_iterations.  A stopped problem's h is latched.
``dtype`` is float64 or ``np.longdouble``; ``perm`` permutes the features (another summation order over v, same
mathematics); ``schedule`` forces each problem's stop iteration instead of testing; ``free_run`` latches nothing and
records every test's relative change and every test's objective for every problem.
"""

from types import SimpleNamespace

import numpy as np

from _refit_ref import EPSILON, normalize, start  # noqa: F401  (normalize is part of this module's interface)


def _wh(h, W):
    return np.einsum("pk,kv->pv", h, W)


def step(x, W, h, al):
    p = _wh(h, W)
    a = x / p
    b = (x + al) / (p + al)
    return np.maximum(h * np.einsum("pv,kv->pk", a, W) / np.einsum("pv,kv->pk", b, W), h.dtype.type(EPSILON))


def objective(x, W, h, al):
    p = _wh(h, W)
    return (x * np.log(x / p) - (x + al) * np.log((x + al) / (p + al))).sum(axis=1)


def objective_scale(x, W, h, al):
    """What the objective's rounding is relative to: the magnitudes of its terms, (x + alpha) once more for the rounding of the
    two sums inside the second logarithm (an error of one ulp there is an error of (x + alpha) ulp in the term), and x + p for
    the objective's slope in h (|d objective / d log p| = alpha |x - p| / (p + alpha) <= x + p)."""
    p = _wh(h, W)
    return (np.abs(x * np.log(x / p)) + (x + al) * (np.abs(np.log((x + al) / (p + al))) + 1.0) + x + p).sum(axis=1)


def nb_refit(X, W, alpha, min_iterations=500, max_iterations=10000, conv_test_freq=10, tol=1e-7, dtype=np.float64, perm=None, schedule=None,
             free_run=False):
    X = np.asarray(X, dtype=np.float64)
    W = np.asarray(W, dtype=np.float64)
    if perm is not None:
        X, W = X[:, perm], W[:, perm]
    x = np.maximum(X, EPSILON).astype(dtype)
    W = W.astype(dtype)
    P, K = x.shape[0], W.shape[0]
    al = np.broadcast_to(np.asarray(alpha, dtype=np.float64), (P,)).astype(dtype).reshape(P, 1)
    h = start(x, K)
    stopped = np.zeros(P, dtype=bool)
    nit = np.zeros(P, dtype=np.int64)
    conv = np.zeros(P, dtype=bool)
    err = np.zeros(P, dtype=dtype)
    prev = objective(x, W, h, al)
    err[:] = prev
    changes, tests, objectives = [], [], [prev.copy()]
    last = int(max_iterations if schedule is None else np.max(schedule))
    if schedule is not None:
        schedule = np.asarray(schedule, dtype=np.int64)
        stopped = schedule == 0
    for it in range(1, last + 1):
        if stopped.all():
            break
        h = np.where(stopped[:, None], h, step(x, W, h, al))
        at_test = it % conv_test_freq == 0
        if schedule is not None:
            now = ~stopped & (schedule == it)
            if now.any():
                cur = objective(x, W, h, al)
                err[now], nit[now] = cur[now], it
                stopped |= now
            continue
        if not (at_test or it == max_iterations):
            continue
        cur = objective(x, W, h, al)
        live = ~stopped
        if at_test:
            with np.errstate(invalid="ignore", divide="ignore"):
                rel = np.abs(prev - cur) / np.abs(prev)
            if free_run:
                changes.append(rel.copy())
                tests.append(it)
                objectives.append(cur.copy())
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
        err = objective(x, W, h, al)
    return SimpleNamespace(exposures=h, reconstruction_errors=err, n_iterations=nit, converged=conv, alpha=al[:, 0], x=x, W=W,
                           changes=np.array(changes).reshape(len(tests), P), tests=np.array(tests, dtype=np.int64), objectives=np.array(objectives))


def constant(X, alpha):
    """c(x, alpha) = sum_v lgamma(x + a) - lgamma(a) - lgamma(x + 1) + x log x - (x + a) log(x + a) + a log a on the clipped x,
    float64: a row's log-likelihood is -divergence + c."""
    from scipy.special import gammaln

    x = np.maximum(np.asarray(X, dtype=np.float64), EPSILON)
    a = np.broadcast_to(np.asarray(alpha, dtype=np.float64), (x.shape[0],)).reshape(-1, 1)
    xa = x + a
    return (gammaln(xa) - gammaln(a) - gammaln(x + 1.0) + x * np.log(x) - xa * np.log(xa) + a * np.log(a)).sum(axis=1)


def poisson_constant(X):
    from scipy.special import gammaln

    x = np.maximum(np.asarray(X, dtype=np.float64), EPSILON)
    return (x * np.log(x) - x - gammaln(x + 1.0)).sum(axis=1)


def _lgamma_ratio_ld(x, a):
    """lgamma(x + a) - lgamma(a) = sum_{j < x} log(a + j) for integer x >= 0, in longdouble (no library lgamma needed)."""
    x = np.asarray(x, dtype=np.int64)
    out = np.zeros(x.shape, dtype=np.longdouble)
    a = np.broadcast_to(np.asarray(a, dtype=np.longdouble), x.shape)
    for j in range(int(x.max(initial=0))):
        out += np.where(j < x, np.log(a + np.longdouble(j)), np.longdouble(0))
    return out


def nbinom_logpmf_ld(X, alpha, p):
    """sum_v log NB(x_v; alpha, alpha / (alpha + p_v)) for INTEGER counts, in longdouble:
    lgamma(x + a) - lgamma(a) - lgamma(x + 1) + a log(a / (a + p)) + x log(p / (a + p))."""
    x = np.asarray(X, dtype=np.int64)
    a = np.broadcast_to(np.asarray(alpha, dtype=np.longdouble), (x.shape[0],)).reshape(-1, 1)
    p = np.asarray(p, dtype=np.longdouble)
    xl = x.astype(np.longdouble)
    return (_lgamma_ratio_ld(x, a) - _lgamma_ratio_ld(x, np.longdouble(1)) + a * np.log(a / (a + p)) + xl * np.log(p / (a + p))).sum(axis=1)


def gamma_poisson_catalogue(N, K, V=96, seed=0, mu=2000.0, alpha=None):
    """(counts (N, V), signatures (K, V), means (N, V)): Dirichlet signatures and exposure shares, `mu` mutations per sample on
    average, and per entry a gamma mixing step of shape `alpha` and mean 1 in front of the Poisson draw (alpha None: Poisson)."""
    rng = np.random.default_rng(seed)
    S = normalize(rng.dirichlet(np.full(V, 0.15), size=K))
    E = rng.dirichlet(np.full(K, 0.5), size=N) * rng.uniform(0.5 * mu, 1.5 * mu, size=(N, 1))
    M = E @ S
    lam = M if alpha is None else M * rng.gamma(alpha, 1.0 / alpha, size=M.shape)
    return rng.poisson(lam).astype(np.float64), S, M


# Recorded on the CPU on the tests' own inputs (tests/test_nb_ref_host.py asserts that they bound what it
# measures, tests/test_gpu_nb_refit.py holds the device to 16 x them)
H_SPREAD = 4.7e-14  # measured 4.63e-14 at (K, V) = (65, 95): largest |dH| / max(H_ld, EPSILON), float64 replica (two feature orders) against longdouble, T = 200
D_SPREAD = 4.6e-17  # measured 4.58e-17 at (33, 17): largest |d objective| / objective_scale, same replicas
G_RAW = 5.5e-4      # measured 5.42e-4 at K = 24 (4.41e-4 at K = 8; problems at alpha = 1e6, where float64's rounding of (x + alpha) / (p + alpha) is 4e-11 of the objective): largest |change - change_ld| / max(change_ld, tol), same replicas, eligible tests up to each problem's stop
MARGIN = 16         # the family's margin ("Accuracy")

ALPHAS = (0.5, 20.0, 1e4, 1e6)
# (K, V): the edges of every KT and short feature axes
FIXED_CASES = [(1, 96), (3, 96), (16, 96), (17, 33), (33, 17), (64, 95), (65, 95), (96, 96)]
FIXED_N, FIXED_T = 40, 200  # two full tiles and a partial one
GRID = np.geomspace(1, 1e4, 17)
# dispersion recovery: gamma-Poisson data with true alpha = 20 (RECOVERY_SEED) and Poisson data from the same means
RECOVERY = dict(N=64, K=4, V=96, mu=2000.0, alpha=20.0)
RECOVERY_SEED = 0


def catalogue(N, K, V=96, seed=0):
    """Poisson counts with three zero-heavy rows, one row with a single mutation and one all-zero row (tests/test_gpu_refit.py's)."""
    from _refit_ref import poisson_catalogue

    X, W = poisson_catalogue(N, K, V=V, seed=seed, zero_heavy=min(3, N - 1))
    if N > 4:
        X[1] = 0.0
        X[1, V // 2] = 1.0
        X[2] = 0.0
    return X, W


def mixed_alpha(N):
    """ALPHAS in turn, so that every tile holds all four"""
    return np.asarray(ALPHAS)[np.arange(N) % len(ALPHAS)]


def entry_dev(H, H_ref):
    H_ref = np.asarray(H_ref, dtype=np.longdouble)
    return float((np.abs(H - H_ref) / np.maximum(H_ref, EPSILON)).max())


def objective_dev(err, ld):
    """|err - err_ld| / objective_scale, the largest over the problems; ld is a longdouble nb_refit result"""
    scale = objective_scale(ld.x, ld.W, ld.exposures, ld.alpha.reshape(-1, 1))
    return float((np.abs(np.asarray(err, dtype=np.longdouble) - ld.reconstruction_errors) / scale).max())


def fixed_case(K, V):
    """(X, W, alpha, keywords) of one fixed-step case"""
    X, W = catalogue(FIXED_N, K, V, seed=K + V)
    return X, W, mixed_alpha(FIXED_N), dict(min_iterations=FIXED_T, max_iterations=FIXED_T)


def host_spread(X, W, alpha, **kw):
    """(longdouble replica, largest entry deviation of H, largest objective deviation) of the float64 replica in two feature orders"""
    perm = np.random.default_rng(7).permutation(X.shape[1])
    ld = nb_refit(X, W, alpha, dtype=np.longdouble, **kw)
    a = nb_refit(X, W, alpha, **kw)
    b = nb_refit(X, W, alpha, perm=perm, **kw)
    return (ld, max(entry_dev(a.exposures, ld.exposures), entry_dev(b.exposures, ld.exposures)),
            max(objective_dev(a.reconstruction_errors, ld), objective_dev(b.reconstruction_errors, ld)))


CONVERGENCE_CASES = [(48, 8), (32, 24)]  # (N, K) at the default stopping rule
CONVERGENCE_KW = dict(min_iterations=500, max_iterations=4000, conv_test_freq=10, tol=1e-7)


def convergence_case(N, K):
    X, W = catalogue(N, K, seed=100 + K)
    return X, W, mixed_alpha(N)


def free_runs(X, W, alpha, last, kw=CONVERGENCE_KW):
    """The longdouble replica and the float64 replica in two feature orders, none of them latching, up to iteration `last`"""
    kw = {**kw, "max_iterations": int(last)}
    perm = np.random.default_rng(7).permutation(X.shape[1])
    return {name: nb_refit(X, W, alpha, free_run=True, **kw, **extra)
            for name, extra in (("ld", dict(dtype=np.longdouble)), ("a", {}), ("b", dict(perm=perm)))}


def change_deviation(free, last, kw=CONVERGENCE_KW):
    """(g_raw, ld_stop): the largest deviation of the float64 replicas' relative change from the longdouble one's, relative to
    max(change, tol), over every eligible test up to the longdouble replica's own stop; and that stop per problem"""
    ld = free["ld"]
    tests, tol = ld.tests, kw["tol"]
    eligible = tests >= kw["min_iterations"]
    P = ld.changes.shape[1]
    ld_stop = np.array([next((t for t, c in zip(tests[eligible], ld.changes[eligible, p]) if c < tol), last) for p in range(P)])
    g_raw = 0.0
    for p in range(P):
        m = eligible & (tests <= ld_stop[p])
        for name in ("a", "b"):
            g_raw = max(g_raw, float((np.abs(free[name].changes[m, p] - ld.changes[m, p]) / np.maximum(ld.changes[m, p], tol)).max(initial=0.0)))
    return g_raw, ld_stop


def schedule_spread(X, W, alpha, nit, kw=CONVERGENCE_KW):
    """The longdouble replica forced to the stop schedule `nit`, and the float64 replicas' largest deviation from it."""
    perm = np.random.default_rng(7).permutation(X.shape[1])
    forced = nb_refit(X, W, alpha, dtype=np.longdouble, schedule=nit, **kw)
    return forced, max(entry_dev(nb_refit(X, W, alpha, schedule=nit, **kw).exposures, forced.exposures),
                       entry_dev(nb_refit(X, W, alpha, schedule=nit, perm=perm, **kw).exposures, forced.exposures))


def recovery_data(poisson=False):
    r = RECOVERY
    X, W, _ = gamma_poisson_catalogue(r["N"], r["K"], r["V"], seed=RECOVERY_SEED, mu=r["mu"], alpha=None if poisson else r["alpha"])
    return X, W


def dispersion_profile(X, W, grid, dtype=np.float64, **kw):
    """What estimate_dispersion computes, on the host: (profile (A, N), poisson log-likelihood (N,), fits)."""
    import _refit_ref

    X = np.asarray(X, dtype=np.float64)
    N, A = X.shape[0], len(grid)
    fit = nb_refit(np.tile(X, (A, 1)), W, np.repeat(np.asarray(grid, dtype=np.float64), N), dtype=dtype, **kw)
    div = np.asarray(fit.reconstruction_errors, dtype=np.float64).reshape(A, N)
    profile = np.stack([-div[a] + constant(X, grid[a]) for a in range(A)])
    pois = _refit_ref.refit(X, W, dtype=dtype, **kw)
    return profile, -np.asarray(pois.reconstruction_errors, dtype=np.float64) + poisson_constant(X), fit


def select(grid, profile, poisson_ll, per_sample=False):
    grid = np.asarray(grid, dtype=np.float64)
    if per_sample:
        best = np.argmax(profile, axis=0)
        return grid[best], best == grid.size - 1, 2.0 * (profile[best, np.arange(profile.shape[1])] - poisson_ll)
    total = profile.sum(axis=1)
    best = int(np.argmax(total))
    return float(grid[best]), best == grid.size - 1, float(2.0 * (total[best] - np.sum(poisson_ll)))
