"""TEST INFRASTRUCTURE ONLY.  The contract of ``sal.exposure_covariance`` on the host.

Per sample, with x = max(row, EPSILON), h the exposures as supplied, A the active signatures and W (K, V) the normalised
signatures (the rows as passed, divided by their sums in float64 as the call does):
    p_v = max(sum_k W[k, v] h_k, EPSILON)  over all k;   d_v = x_v / p_v^2 ("observed") or 1 / p_v ("expected")
    J[k, l] = sum_v W[k, v] W[l, v] d_v  on A;   C = D^-1/2 J D^-1/2, D = diag(J);   C = L L^T, natural order, no pivoting
    singular at the first squared pivot <= min_pivot;  min_pivot_value = the smallest squared pivot up to there
    inflation = diag(C^-1);  standard_errors = sqrt(inflation / diag(J));  corr = C^-1 scaled to a unit diagonal

:func:`reference` evaluates it in ``np.longdouble`` (x87 extended, 64-bit mantissa) as ``tests/_corr_ref.py`` does: a 96 x 96
factorisation per sample in mpmath would take minutes per test, so mpmath (50 digits) checks the long-double code itself, on
small problems, in ``tests/test_cov_host.py``.  A squared pivot of the reference below ``PIVOT_NOISE`` -- 64 K eps of the long
double, what its own rounding can leave of an exact zero -- is reported as exactly 0.0: the reference cannot tell it from 0.

:func:`replica` is the same contract in float64 in two evaluation orders each for its two stages: J summed over the features
ascending or descending, the inverse from the Cholesky factor or from ``np.linalg.inv``.  The distance of the four replicas from
the reference is what a float64 evaluation of the contract may differ by on given inputs (``measure``).

The input builders are seeded: Dirichlet signatures with Poisson counts (``poisson_case``), a confounded case, a case with an
exactly duplicated signature, and exposures with exact zeros (``restrict_support``).
"""

from types import SimpleNamespace

import numpy as np

EPSILON = float(np.finfo(np.float32).eps)
LD = np.longdouble
assert np.finfo(LD).eps < 2e-19, "np.longdouble is not an extended type on this platform"

FIELDS = ("standard_errors", "inflation", "information_diag")  # compared relatively; correlations absolutely


def normalize(S):
    S = np.ascontiguousarray(S, dtype=np.float64)
    return np.ascontiguousarray(S / S.sum(axis=1, keepdims=True))


def default_active(H):
    return np.asarray(H) > 0.0


def _weights(x, W, h, information, dtype):
    x = np.maximum(x.astype(dtype), dtype(EPSILON))
    p = np.maximum(h.astype(dtype) @ W.astype(dtype), dtype(EPSILON))
    return x / (p * p) if information == "observed" else dtype(1.0) / p


def _information(Wa, d, order):
    """J = Wa diag(d) Wa^T, one feature after the other in the given order"""
    J = np.zeros((Wa.shape[0], Wa.shape[0]), dtype=d.dtype)
    features = range(Wa.shape[1]) if order == "ascending" else range(Wa.shape[1] - 1, -1, -1)
    for v in features:
        J += d[v] * np.outer(Wa[:, v], Wa[:, v])
    return J


def _cholesky(C, min_pivot, noise):
    """Right-looking, in the natural order -> (L, smallest squared pivot up to the first one <= min_pivot, singular)"""
    A = C.copy()
    n = A.shape[0]
    L = np.zeros_like(A)
    smallest = A.dtype.type(np.inf)
    for j in range(n):
        piv = A[j, j]
        if abs(piv) < noise:
            piv = A.dtype.type(0.0)
        if not piv > min_pivot:
            return L, piv, True
        smallest = min(smallest, piv)
        L[j, j] = np.sqrt(piv)
        L[j + 1:, j] = A[j + 1:, j] / L[j, j]
        A[j + 1:, j + 1:] -= np.outer(L[j + 1:, j], L[j + 1:, j])
    return L, smallest, False


def _invert_lower(L):
    n = L.shape[0]
    X = np.zeros_like(L)
    for i in range(n):
        X[i, i] = L.dtype.type(1.0) / L[i, i]
        if i:
            X[i, :i] = -(L[i, :i] @ X[:i, :i]) / L[i, i]
    return X


def _evaluate(X, W, H, active, information, min_pivot, dtype, order, inverse, noise):
    X, W, H = np.asarray(X, dtype=np.float64), normalize(W), np.asarray(H, dtype=np.float64)  # (the call normalises what it is given)
    N, K = H.shape
    active = default_active(H) if active is None else np.broadcast_to(np.asarray(active, dtype=bool), (N, K))
    out = SimpleNamespace(
        standard_errors=np.full((N, K), np.nan, dtype=dtype), inflation=np.full((N, K), np.nan, dtype=dtype),
        information_diag=np.full((N, K), np.nan, dtype=dtype), max_abs_correlation=np.full((N, K), np.nan, dtype=dtype),
        most_confounded=np.full((N, K), -1, dtype=np.int32), gap=np.full((N, K), np.nan, dtype=dtype),
        min_pivot_value=np.full(N, np.nan, dtype=dtype), singular=np.zeros(N, dtype=bool), n_active=active.sum(axis=1).astype(np.int32),
        correlation=np.full((N, K, K), np.nan, dtype=dtype), active=active)
    for n in range(N):
        idx = np.flatnonzero(active[n])
        if idx.size == 0:
            continue
        d = _weights(X[n], W, H[n], information, dtype)
        J = _information(W[idx].astype(dtype), d, order)
        D = np.diag(J).copy()
        C = J / np.sqrt(np.outer(D, D))
        np.fill_diagonal(C, dtype(1.0))
        L, out.min_pivot_value[n], out.singular[n] = _cholesky(C, dtype(min_pivot), noise)
        if out.singular[n]:
            continue
        if inverse == "cholesky":
            Li = _invert_lower(L)
            Ci = Li.T @ Li
        else:
            Ci = np.linalg.inv(C)
        v = np.diag(Ci).copy()
        corr = Ci / np.sqrt(np.outer(v, v))
        corr = np.tril(corr) + np.tril(corr, -1).T  # one number per unordered pair
        np.fill_diagonal(corr, dtype(1.0))
        out.inflation[n, idx], out.information_diag[n, idx] = v, D
        out.standard_errors[n, idx] = np.sqrt(v / D)
        out.correlation[n][np.ix_(idx, idx)] = corr
        if idx.size > 1:
            off = np.abs(corr)
            np.fill_diagonal(off, dtype(-1.0))
            best = off.argmax(axis=1)  # (the first of equal values)
            out.most_confounded[n, idx] = idx[best]
            out.max_abs_correlation[n, idx] = off[np.arange(idx.size), best]
            ranked = np.sort(off, axis=1)
            out.gap[n, idx] = ranked[:, -1] - ranked[:, -2] if idx.size > 2 else np.inf
    return out


def reference(X, W, H, active=None, information="observed", min_pivot=1e-10):
    """The contract in long double.  ``gap`` is the distance between the two largest |corr| of a row (inf with one partner)."""
    K = np.asarray(H).shape[1]
    return _evaluate(X, W, H, active, information, min_pivot, LD, "ascending", "cholesky", 64.0 * K * float(np.finfo(LD).eps))


def replica(X, W, H, active=None, information="observed", min_pivot=1e-10, order="ascending", inverse="cholesky"):
    """The contract in float64; ``order`` of the features in J, ``inverse`` from the Cholesky factor or ``np.linalg.inv``"""
    return _evaluate(X, W, H, active, information, min_pivot, np.float64, order, inverse, 0.0)


REPLICAS = (("ascending", "cholesky"), ("descending", "cholesky"), ("ascending", "inv"), ("descending", "inv"))


def deviation(got, ref):
    """-> (largest |got - ref| / ref over the three relative fields, largest absolute difference of the correlations and of the
    smallest pivots), over the entries the reference defines; the NaN patterns must agree."""
    rel = 0.0
    for name in FIELDS:
        g, r = np.asarray(getattr(got, name), dtype=LD), np.asarray(getattr(ref, name), dtype=LD)
        assert np.array_equal(np.isnan(g), np.isnan(r)), name
        ok = ~np.isnan(r)
        if ok.any():
            rel = max(rel, float((np.abs(g[ok] - r[ok]) / np.abs(r[ok])).max()))
    absolute = 0.0
    live = ~np.asarray(ref.singular)  # (a singular sample's pivot is whatever rounding leaves of a zero)
    pairs = [(got.max_abs_correlation, ref.max_abs_correlation), (np.asarray(got.min_pivot_value)[live], np.asarray(ref.min_pivot_value)[live])]
    if getattr(got, "correlation", None) is not None:
        pairs.append((got.correlation, ref.correlation))
    for g, r in pairs:
        g, r = np.asarray(g, dtype=LD), np.asarray(r, dtype=LD)
        assert np.array_equal(np.isnan(g), np.isnan(r))
        ok = ~np.isnan(r)
        if ok.any():
            absolute = max(absolute, float(np.abs(g[ok] - r[ok]).max()))
    return rel, absolute


def measure(X, W, H, active=None, information="observed", min_pivot=1e-10, ref=None):
    """The four float64 replicas' largest deviation from the reference -> (relative, absolute)"""
    ref = reference(X, W, H, active, information, min_pivot) if ref is None else ref
    rel, absolute = 0.0, 0.0
    for order, inverse in REPLICAS:
        r, a = deviation(replica(X, W, H, active, information, min_pivot, order, inverse), ref)
        rel, absolute = max(rel, r), max(absolute, a)
    return rel, absolute


# ---- inputs

def signatures(K, V, seed=0):
    """K signatures over V features: half of each one's mass on a feature of its own (k mod V), half Dirichlet(0.3) -- distinct
    enough for a well-conditioned information matrix wherever at most V of them are active"""
    rng = np.random.default_rng([seed, K, V])
    W = 0.5 * rng.dirichlet(np.full(V, 0.3), size=K)
    W[np.arange(K), np.arange(K) % V] += 0.5
    return normalize(W)


def poisson_case(N, K, V, seed=0, mutations=(200, 20000), W=None):
    """-> (X counts, W, H exposures): Poisson counts of N samples with Dirichlet loads on the K signatures; H is the generating
    exposures times a lognormal factor, standing for a fit (the contract takes any exposures)"""
    rng = np.random.default_rng([seed, N, K, V, 1])
    W = signatures(K, V, seed) if W is None else W
    total = np.exp(rng.uniform(np.log(mutations[0]), np.log(mutations[1]), size=N))
    E = total[:, None] * rng.dirichlet(np.full(K, 0.5), size=N)
    X = rng.poisson(E @ W).astype(np.float64)
    H = np.maximum(E * np.exp(rng.normal(0.0, 0.2, size=E.shape)), EPSILON)
    return X, W, H


def subset_mask(N, K, size, seed=0, full=()):
    """(N, K) bool: `size` signatures with distinct k mod size per sample (at most K); the rows in `full` keep all K"""
    rng = np.random.default_rng([seed, N, K, 2])
    A = np.zeros((N, K), dtype=bool)
    for n in range(N):
        A[n, rng.permutation(K)[: min(size, K)]] = True
    A[list(full)] = True
    return A


def confounded_case(N, K, V, seed=0, mixed=2, parents=(0, 1)):
    """Signature `mixed` is 0.98 a + 0.02 b of the signatures `parents` = (a, b), renormalised.  b stays in the catalogue but carries
    no exposure, so it is inactive by default: with a, b and their mixture all active the matrix would be singular exactly"""
    W = signatures(K, V, seed)
    W[mixed] = 0.98 * W[parents[0]] + 0.02 * W[parents[1]]
    X, W, H = poisson_case(N, K, V, seed, W=normalize(W))
    H[:, parents[1]] = 0.0
    return X, W, H


def duplicate_case(N, K, V, seed=0, copy=2, of=0):
    """Signature `copy` is signature `of`, bit for bit: every sample with both active is singular"""
    W = signatures(K, V, seed)
    W[copy] = W[of]
    return poisson_case(N, K, V, seed, W=W)


def restrict_support(H, keep, seed=0):
    """H with exact zeros: every sample keeps `keep` of its signatures, chosen at random"""
    rng = np.random.default_rng([seed, 3])
    out = np.zeros_like(H)
    for n in range(H.shape[0]):
        idx = rng.permutation(H.shape[1])[: min(keep, H.shape[1])]
        out[n, idx] = H[n, idx]
    return out


# ---- the device tests' inputs (tests/test_gpu_covariance.py; tests/test_cov_host.py measures the tolerances on them)

GPU_N = 40
GPU_SHAPES = tuple((K, V) for K in (1, 3, 16, 17, 64, 96) for V in (7, 96))


def gpu_case(K, V, seed=0):
    """-> (X, W, H, active) for N = 40.  With K <= V every signature is active, except that samples 5 and 6 keep half of their
    support (exact zeros in H) and sample 7 has no exposure at all; with K > V = 7 a sample's active set is 5 signatures, and
    samples 0 and 1 keep all K: rank deficient, so singular.  From K = 64 on the samples carry 2e5 to 2e6 mutations: a feature
    without a count has next to no weight in the observed information, and with about as many signatures as features every such
    feature costs the matrix a dimension."""
    X, W, H = poisson_case(GPU_N, K, V, seed, mutations=(200, 20000) if K < 64 else (2e5, 2e6))
    if K <= V:
        H[5:7] = restrict_support(H[5:7], max(1, K // 2), seed)
        H[7] = 0.0
        return X, W, H, default_active(H)
    return X, W, H, subset_mask(GPU_N, K, 5, seed, full=(0, 1))
