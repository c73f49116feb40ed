"""Host replicas and input generators for the device-side initialisation (``csrc/salnmf_init_kernels.h``,
``csrc/salnmf_host_init.h``, ``device_init.py``); no device code.  Used by ``test_init_ref_host.py`` (CPU) and
``test_gpu_init_entrywise.py`` (MI355X).  DESIGN.md 8.2 has the table of comparisons.

Three kinds of comparison:

* **exact** -- inputs on which the true result is a float64 and every partial sum in any order is one too (integer counts,
  B in sixteenths, one-hot rows): a correct kernel returns the same bits whatever its summation order, so the tests use
  ``np.array_equal``.  The premises (largest magnitudes, bit budgets) are functions here and asserted on the CPU.
* **derived bound** -- Poisson counts clipped to EPSILON and a B from the case's own ``eigh``: every entry of the projection
  against ``numpy.longdouble`` within ``(V + 2) 2^-53 a_nj``, ``a_nj = sum_v |x_nv| |b_jv|`` (V fused multiply-adds, each
  rounding at most half an ulp of a partial sum that ``a`` bounds), the norms within the bound that follows from it.
* **measured spread x 16** -- the winning norms of the separable selection: the float64 replica in two feature orders
  against the long-double replica, measured per case on the CPU, the largest recorded in the GPU test file.

Layouts are the engine's: ``X (N, V)``, ``B (K, V)``, ``H (N, K)``.
"""

from __future__ import annotations

import numpy as np

EPSILON = float(np.finfo(np.float32).eps)
EPS64 = 2.0**-53
L = np.longdouble
ZERO_BELOW = 1e-6  # sklearn's eps of _initialize_nmf
VMAX, KC = 96, 64  # features per block, signatures per chunk (salnmf_kernels.h, salnmf.hip)

GRAM_SHAPES = [(1, 1), (16, 96), (37, 83), (37, 7), (37, 97), (37, 192), (21, 250)]
PROJECT_SHAPES = [(37, 96, 1), (37, 96, 16), (37, 96, 17), (37, 83, 5), (37, 97, 5), (21, 250, 7), (37, 96, 65), (37, 96, 130), (21, 192, 70)]
# 16 405 samples are 1 026 tiles of 16: more than the 1 024 workgroups init_project / init_separable launch at most, more than
# the 16 384 rows one sweep of init_flat's 1 024 x 256 threads covers (16 lanes per row), and -- see MANY_TILES_N -- more than
# the waves of the Gram launch
MANY_ROWS = 16405
FLAT_SHAPES = [(37, 83, 5), (21, 250, 70), (MANY_ROWS, 96, 3)]
FINISH_SHAPES = [(96, 5), (96, 17), (96, 70), (250, 5), (250, 70)]  # (V = N, K)
WHOLE_CASES = [(96, 203, 16, "nndsvd"), (83, 77, 7, "nndsvda"), (96, 300, 80, "nndsvd"), (250, 150, 70, "nndsvda")]
SEPARABLE_SHAPES = [(40, 7, 5), (777, 83, 12), (203, 96, 30), (150, 250, 10), (60, 97, 4)]

# The Gram launch (salnmf.hip: salnmf_create) has grid = min(compute units, ceil(tiles / 4)) workgroups of four waves, one
# 16-sample tile per wave and round.  The MI355X has 256 compute units: 1 024 waves, so from tile 1 025 on (N > 16 384) a wave
# accumulates a second tile.  16 405 samples are 1 026 tiles: waves 0 and 1 of workgroup 0 take two, the last one ragged.  (On
# a device with fewer units the same N only gives more waves a second tile.)
MANY_TILES_N = MANY_ROWS


def chunk_starts(K):
    """First global column of every signature chunk (salnmf.hip: salnmf_create -- chunks of equal size ceil(K / NC), NC =
    ceil(K / 64)); [0] for K <= 64.  K = 70: [0, 35]; K = 130: [0, 44, 88]."""
    nc = (K + KC - 1) // KC
    ck = (K + nc - 1) // nc
    return [c * ck for c in range(nc)]


# ------------------------------------------------------------------------------------------ (1) exact-arithmetic inputs
def count_matrix(N, V, seed=0):
    """int64 counts in [0, 255], about 30 % zeros; sample N // 2 all zero (N >= 3), the last sample with all its mass in the
    last feature (N >= 2; for N = 1 the only sample is an ordinary one)."""
    rng = np.random.default_rng(1000 * N + V + seed)
    X = rng.integers(1, 256, size=(N, V))
    X[rng.random((N, V)) < 0.3] = 0
    if N >= 3:
        X[N // 2] = 0
    if N >= 2:
        X[N - 1] = 0
        X[N - 1, V - 1] = 255
    return X.astype(np.int64)


def gram_exact(Xi):
    """(X^T X, sum of X) in int64"""
    Xi = np.asarray(Xi, dtype=np.int64)
    return Xi.T @ Xi, int(Xi.sum())


def sixteenths(K, V, seed=0):
    """B (K, V) with entries k / 16, k an integer in [-16, 16], and the int64 numerators; row K // 2 all zero (K >= 3), the
    last row zero outside the last feature block (K >= 2; with V <= 96 that block is the whole row)."""
    rng = np.random.default_rng(77 * K + V + seed)
    Bi = rng.integers(-16, 17, size=(K, V)).astype(np.int64)
    if K >= 3:
        Bi[K // 2] = 0
    if K >= 2:
        Bi[K - 1, : VMAX * ((V - 1) // VMAX)] = 0
    return Bi / 16.0, Bi


def project_exact(Xi, Bi):
    """U = X B^T, pos2, neg2 for B = Bi / 16 from integer arithmetic: (U, pos2, neg2, bits) with ``bits`` the largest
    number of bits any partial sum can need (|U| 16 and the column sums of U^2 256, both integers)."""
    U16 = np.asarray(Xi, dtype=np.int64) @ np.asarray(Bi, dtype=np.int64).T
    A16 = np.asarray(Xi, dtype=np.int64) @ np.abs(np.asarray(Bi, dtype=np.int64)).T  # bounds every partial sum of a chain
    p = (np.maximum(U16, 0) ** 2).sum(axis=0)
    m = (np.minimum(U16, 0) ** 2).sum(axis=0)
    # (the device adds positive and negative parts apart; any partial sum of non-negative terms is below the column's total)
    bits = max(int(A16.max()).bit_length(), int((U16**2).sum(axis=0).max()).bit_length())
    return U16 / 16.0, p / 256.0, m / 256.0, bits


def flat_post(K, X, seed=0):
    """column factors: every third sends every entry below EPSILON, every fourth about half of them (the samples whose row sum
    is below the median), the rest none but the all-zero sample's"""
    rng = np.random.default_rng(K + seed)
    post = rng.uniform(0.5, 2.0, K)
    post[1::4] = EPSILON * K / float(np.median(np.asarray(X).sum(axis=1)))
    post[::3] = 1e-12
    return post


def flat_replica(X, post, Ktot=None):
    """init_flat_kernel: rowsum / Ktot * post[j], max with EPSILON -- one division, one product (float64, as the kernel)"""
    X = np.asarray(X, dtype=np.float64)
    e = X.sum(axis=1) / (len(post) if Ktot is None else Ktot)
    v = e[:, None] * np.asarray(post, dtype=np.float64)[None, :]
    return np.where(v < EPSILON, EPSILON, v)


def finish_replica(U, scale, take_neg, post, zero_below, fill, first_cols=(0,), dtype=None):
    """init_finish_kernel per element, in ``U``'s precision (float64 reproduces the kernel bit for bit; long double is the
    reference of part 3).  ``first_cols``: the columns that take |x| -- global column 0 only."""
    U = np.asarray(U) if dtype is None else np.asarray(U).astype(dtype)
    t = U.dtype.type
    scale, post = np.asarray(scale, dtype=np.float64).astype(U.dtype), np.asarray(post, dtype=np.float64).astype(U.dtype)
    neg = np.asarray(take_neg).astype(bool)[None, :]
    part = np.where(neg, np.where(U < 0, -U, t(0)), np.where(U > 0, U, t(0)))
    v = scale[None, :] * part
    for j in first_cols:
        v[:, j] = np.abs(U[:, j]) * scale[j]
    v[v < t(zero_below)] = t(0)
    if fill != 0.0:
        v[v == 0] = t(fill)
    out = v * post[None, :]
    return np.where(out < t(EPSILON), t(EPSILON), out)


def _step(v, d):
    for _ in range(abs(d)):
        v = float(np.nextafter(v, np.inf if d > 0 else -np.inf))
    return v


def _solve(target, factor, start):
    """a positive double x near ``start`` with fl(factor(x)) == target, or None"""
    for d in (0, 1, -1, 2, -2, 3, -3, 4, -4):
        x = _step(start, d)
        if factor(x) == target:
            return x
    return None


def finish_case(V, K, seed=0):
    """Probes of init_finish_kernel through the production hand-over.  Returns (X one-hot int64 (V, V), B (K, V), scale,
    take_neg, post, perm).  Sample n has its single 1 at feature perm[n], so ``init_project(B)`` leaves H[n, j] = B[j, perm[n]]
    exactly.  Column j's probes, each with both signs: 0, the values whose scaled part is ZERO_BELOW and one ulp to either
    side, the values whose product with post[j] is EPSILON and one ulp to either side, far below both, a subnormal, large
    values.  Scales and posts are powers of two in most columns (the exact hits then exist by construction), arbitrary in the
    others (found by search where they exist).  take_neg alternates, and is 0 with negative probes present in column 0, in
    the first column of every chunk after the first and in column 64: those must become the fill or the floor, never |x|."""
    rng = np.random.default_rng(V + K + seed)
    scales = [1.0, 0.5, 4.0, 1.3719, 0.125, 0.7301]
    posts = [1.0, 2.0**-4, 3.7, 2.0**-6, 0.81]
    scale = np.array([scales[j % len(scales)] for j in range(K)])
    post = np.array([posts[j % len(posts)] for j in range(K)])
    take_neg = (np.arange(K) % 2).astype(np.int32)
    for j in set(chunk_starts(K)) | ({64} if K > 64 else set()):
        take_neg[j] = 0
    B = np.zeros((K, V))
    for j in range(K):
        s, p = float(scale[j]), float(post[j])
        xz = _solve(ZERO_BELOW, lambda x: s * x, ZERO_BELOW / s) or ZERO_BELOW / s
        xe = _solve(EPSILON, lambda x: (s * x) * p, EPSILON / p / s) or EPSILON / p / s
        mags = [0.0, xz, _step(xz, -1), _step(xz, 1), xe, _step(xe, -1), _step(xe, 1), xz * 1e-3, xe * 1e-3, 5e-324, 2.0**-1040, 3.0, 12345.678,
                2.0**52 + 1.0, 1e150]
        probes = [sg * m for m in mags for sg in (1.0, -1.0)]
        for v in range(V):
            B[j, v] = probes[(v + 7 * j) % len(probes)]
    perm = rng.permutation(V)
    X = np.zeros((V, V), dtype=np.int64)
    X[np.arange(V), perm] = 1
    return X, B, scale, take_neg, post, perm


FINISH_FILLS = (0.0, 0.25, 2.0**-20)  # 2^-20 x post = 2^-4 or 2^-6 lies below EPSILON


# ------------------------------------------------------------------------------------ (2) generic inputs, derived bounds
def generic_case(N, V, K, seed=0):
    """Poisson counts clipped to EPSILON (as fit() hands them over) and B = (eigenvectors / sigma)^T of the case's own Gram
    matrix, as ``initialize_on_device`` forms it.  More rows than eigenvectors (K > V): the rows wrap around, negated."""
    rng = np.random.default_rng(31 * N + V + K + seed)
    X = rng.poisson(rng.gamma(1.0, 20.0, size=(N, V))).astype(np.float64).clip(EPSILON)
    evals, evecs = np.linalg.eigh(X.T @ X)
    order = np.argsort(evals)[::-1][: min(K, V)]
    sigma = np.sqrt(np.maximum(evals[order], 0.0))
    with np.errstate(divide="ignore", invalid="ignore"):
        B = np.nan_to_num((evecs[:, order] / sigma).T, nan=0.0, posinf=0.0, neginf=0.0)
    j = np.arange(K)
    return X, np.ascontiguousarray(B[j % B.shape[0]] * np.where((j // B.shape[0]) % 2 == 1, -1.0, 1.0)[:, None])


def project_ld(X, B):
    """(U, a, pos2, neg2) in long double: the reference of the projection and its error unit a_nj = sum |x| |b|"""
    Xl, Bl = np.asarray(X, dtype=np.float64).astype(L), np.asarray(B, dtype=np.float64).astype(L)
    U = Xl @ Bl.T
    a = np.abs(Xl) @ np.abs(Bl).T
    return U, a, (np.maximum(U, 0) ** 2).sum(axis=0), (np.minimum(U, 0) ** 2).sum(axis=0)


def project_bounds(U, a, N, V):
    """(per entry, per column): |U - U_ld| <= (V + 2) 2^-53 a;  |pos2 - pos2_ld|, |neg2 - neg2_ld| <=
    2^-53 [2 (V + 2) sum_n |U| a + (N + 2) sum_n U^2] -- the error of U passed through the square, and a sum of N non-negative
    terms in any order"""
    bu = (V + 2) * EPS64 * a
    bn = EPS64 * (2 * (V + 2) * (np.abs(U) * a).sum(axis=0) + (N + 2) * (U**2).sum(axis=0))
    return bu, bn


def project_ratios(Ugot, pgot, ngot, U, a, p, n, N, V):
    """(worst entry ratio, worst norm ratio) of a float64 result against the long-double one, each in its bound"""
    bu, bn = project_bounds(U, a, N, V)
    with np.errstate(divide="ignore", invalid="ignore"):
        ru = np.where(bu > 0, np.abs(np.asarray(Ugot).astype(L) - U) / bu, np.where(np.asarray(Ugot) == U, 0, np.inf))
        rn = np.where(bn > 0, np.maximum(np.abs(np.asarray(pgot).astype(L) - p), np.abs(np.asarray(ngot).astype(L) - n)) / bn,
                      np.where((np.asarray(pgot) == p) & (np.asarray(ngot) == n), 0, np.inf))
    return float(ru.max()), float(rn.max())


def project_f64(X, B, reverse=False):
    """NumPy's float64 projection and norms, in ascending or descending feature order"""
    X, B = np.asarray(X, dtype=np.float64), np.asarray(B, dtype=np.float64)
    U = (X[:, ::-1] @ B[:, ::-1].T) if reverse else (X @ B.T)
    return U, (np.maximum(U, 0) ** 2).sum(axis=0), (np.minimum(U, 0) ** 2).sum(axis=0)


# ------------------------------------------------------------------------------- (3) the whole initialize_on_device
def whole_counts(V, N, K, seed=None):
    """int64 counts, not clipped: gamma(0.5, 80) exposures on min(K, 12) Dirichlet(0.3) signatures, seed V + K; sample N // 3
    all zero, sample N - 2 a duplicate of sample 1"""
    rng = np.random.default_rng(V + K if seed is None else seed)
    k0 = min(K, 12)
    Wt = rng.dirichlet(np.full(V, 0.3), size=k0)
    X = rng.poisson(rng.gamma(0.5, 80.0, size=(N, k0)) @ Wt).astype(np.int64)
    X[N // 3] = 0
    X[N - 2] = X[1]
    return X


class WholeHost:
    """The host side of one part-3 case, up to the norms: Gram matrix in int64, ``eigh`` under one BLAS thread, B, U and the
    norms in long double.  ``recipe(pos2, neg2)`` is ``nndsvd_signature_side`` + ``normalize_WH`` as ``initialize_on_device``
    runs them; ``exposures(recipe)`` the finish replica on the long-double U."""

    def __init__(self, V, N, K, method, X=None):
        from salamander_amd.device_init import _single_blas_thread

        self.V, self.N, self.K, self.method = V, N, K, method
        self.X = whole_counts(V, N, K) if X is None else X
        Gi, total = gram_exact(self.X)
        assert int(Gi.max()) < 2**53
        self.G, self.total = Gi.astype(np.float64), float(total)
        with _single_blas_thread():
            evals, evecs = np.linalg.eigh(self.G)
        order = np.argsort(evals)[::-1][:K]
        self.evals, self.evecs = evals[order], evecs[:, order]
        sigma = np.sqrt(np.maximum(self.evals, 0.0))
        with np.errstate(divide="ignore", invalid="ignore"):
            B = (self.evecs / sigma).T
        self.B = np.ascontiguousarray(np.nan_to_num(B, nan=0.0, posinf=0.0, neginf=0.0))
        self.U, self.a, self.pos2, self.neg2 = project_ld(self.X, self.B)
        self.bound_u, self.bound_n = project_bounds(self.U, self.a, N, V)

    def recipe(self, pos2, neg2):
        from salamander_amd.device_init import nndsvd_signature_side

        pos2, neg2 = np.asarray(pos2).astype(np.float64), np.asarray(neg2).astype(np.float64)
        with np.errstate(divide="ignore", invalid="ignore"):
            S_raw, scale, take_neg, fill = nndsvd_signature_side(self.evals, self.evecs, pos2, neg2, self.K, self.total / (self.N * self.V), self.method)
            colsum = S_raw.sum(axis=1)
            S_out = (S_raw / colsum[:, None]).clip(EPSILON)
        return {"S": S_out, "scale": np.nan_to_num(scale, nan=0.0, posinf=0.0), "scale_raw": scale, "take_neg": take_neg, "fill": fill, "post": colsum}

    def exposures(self, r):
        """(replica (N, K) long double, exact mask, bound): the finish replica on the long-double U; ``exact`` marks the entries
        the threshold zeroed (they are the fill-derived value or EPSILON) and those at EPSILON; the others are within
        (V + 4) 2^-53 a scale post."""
        E = finish_replica(self.U, r["scale"], r["take_neg"], r["post"], ZERO_BELOW, r["fill"])
        scaled = self.scaled(r)
        exact = (scaled < L(ZERO_BELOW)) | (E == L(EPSILON))
        bound = (self.V + 4) * EPS64 * self.a * r["scale"][None, :] * r["post"][None, :]
        return E, exact, bound

    def scaled(self, r):
        """the scaled part before the threshold, long double"""
        neg = r["take_neg"].astype(bool)[None, :]
        part = np.where(neg, np.maximum(-self.U, 0), np.maximum(self.U, 0))
        part[:, 0] = np.abs(self.U[:, 0])
        return part * r["scale"].astype(L)[None, :]

    def isolation(self, r, pos2=None, neg2=None):
        """Counts of the discrete decisions a rounding could flip (all have to be 0), and the smallest kept eigenvalue:
        sign    columns j >= 1 with |m_p - m_n| <= 1e-9 max(m_p, m_n)
        thresh  entries whose scaled part is neither 0 nor further than 4 (V + 2) 2^-53 a scale from ZERO_BELOW
        zero    entries with 0 < |U| <= 4 (V + 2) 2^-53 a
        floor   entries above the threshold whose product with post is within the entry's bound of EPSILON"""
        pos2 = self.pos2 if pos2 is None else np.asarray(pos2).astype(L)
        neg2 = self.neg2 if neg2 is None else np.asarray(neg2).astype(L)
        Vt = self.evecs.T
        yp = np.sqrt((np.maximum(Vt, 0) ** 2).sum(axis=1))
        yn = np.sqrt((np.minimum(Vt, 0) ** 2).sum(axis=1))
        mp_, mn_ = np.sqrt(pos2) * yp, np.sqrt(neg2) * yn
        sign = int((np.abs(mp_ - mn_) <= 1e-9 * np.maximum(mp_, mn_))[1:].sum())
        sc = self.scaled(r)
        margin = 4 * (self.V + 2) * EPS64 * self.a
        thresh = int(((sc != 0) & (np.abs(sc - L(ZERO_BELOW)) <= margin * r["scale"][None, :])).sum())
        zero = int(((self.U != 0) & (np.abs(self.U) <= margin)).sum())
        _, _, bound = self.exposures(r)
        fl = int(((sc >= L(ZERO_BELOW)) & (np.abs(sc * r["post"].astype(L)[None, :] - L(EPSILON)) <= bound)).sum())
        return {"sign": sign, "thresh": thresh, "zero": zero, "floor": fl, "finite": bool(np.isfinite(r["scale_raw"]).all()), "min_eval": float(self.evals.min())}


# ---------------------------------------------------------------------------------------- (4) the separable selection
def separable_replica(X, K, dtype=L, reverse=False):
    """The selection loop (methods.py:112-135; sep_pass_kernel / sep_select_kernel): rows normalised to sum 1, K rounds of
    argmax of the squared norms (lowest index on ties) and the deflation R - u (u . R) / |u|^2.  Returns (chosen (K,), winning
    norms (K,), margins (K,)): the relative lead of the winner over the best row that is not a duplicate of it in X."""
    X = np.asarray(X, dtype=np.float64)
    R = X.astype(dtype)
    if reverse:
        R = R[:, ::-1]
    R = R / R.sum(axis=1, keepdims=True)
    chosen, norms, margins = [], [], []
    for _ in range(K):
        nrm = (R * R).sum(axis=1)
        j = int(np.argmax(nrm))
        others = ~(X == X[j]).all(axis=1)
        runner = nrm[others].max() if others.any() else dtype(0)
        chosen.append(j), norms.append(nrm[j]), margins.append(float((nrm[j] - runner) / nrm[j]) if nrm[j] > 0 else 0.0)
        u = R[j].copy()
        R = R - np.outer(R @ u, u) / nrm[j]
    return np.array(chosen), np.array(norms, dtype=dtype), np.array(margins)


def separable_spread(X, K):
    """(long-double replica, largest |norm64 - norm_ld| / norm_ld[0] over both feature orders and all rounds)"""
    ld = separable_replica(X, K, L)
    spread = 0.0
    for rev in (False, True):
        _, n64, _ = separable_replica(X, K, np.float64, rev)
        spread = max(spread, float((np.abs(n64.astype(L) - ld[1]) / ld[1][0]).max()))
    return ld, spread


def separable_counts(N, V, K, seed=None):
    """the existing test's input (oracle synthetic problem: zeros clipped to EPSILON)"""
    from oracle import klnmf_oracle as orc

    X, _, _ = orc.synthetic_problem(V, N, min(K, 8), seed=N if seed is None else seed)
    return X


def rank3_catalogue():
    """400 samples drawn from three distinct rows (test_gpu_init.py's rank-deficient catalogue)"""
    rng = np.random.default_rng(0)
    base = rng.poisson(50.0, size=(3, 96)).astype(float) + 1.0
    return base[rng.integers(0, 3, size=400)]


# row n is handled by workgroup (n mod 16 384) // 16, slot n mod 16; sep_select_kernel's thread t first reduces the workgroups t, t + 256, ...
TIE_ROWS = {
    # round-0 winner at rows r, r + 7 (same workgroup, other slot), r + 16, r + 5000, r + 16400 (the second sweep of r + 16's thread)
    "spread": ((3, 10, 19, 5003, 16403), (40, 56, 9000, 16404)),
    # the lowest copy in workgroup 1023, a higher one in workgroup 0's second sweep: the selection tree compares indices
    "last": ((16370, 16375, 16390), (16371, 16398)),
    # workgroups 0 and 256 (1 and 257) meet in one thread's strided pre-reduction, the later workgroup holding the lower row
    "strided": ((4099, 16387), (4115, 16400)),
}


def tie_case(variant="spread", seed=5):
    """N = 16 405 x V = 96 clipped Poisson counts in which the rows of the largest round-0 norm (all mass in feature 5) and of
    the largest round-1 norm (nearly all mass in feature 50) are repeated at ``TIE_ROWS[variant]``.  Equal rows go through
    identical arithmetic, so the ties are exact.  Returns (X, expected chosen[:2])."""
    rng = np.random.default_rng(seed)
    N, V = MANY_ROWS, 96
    X = rng.poisson(rng.gamma(1.0, 20.0, size=(N, V))).astype(np.float64)
    a = np.zeros(V)
    a[5] = 1000.0
    b = np.zeros(V)
    b[50], b[51] = 1000.0, 10.0
    ia, ib = TIE_ROWS[variant]
    X[list(ia)] = a
    X[list(ib)] = b
    return X.clip(EPSILON), [min(ia), min(ib)]
