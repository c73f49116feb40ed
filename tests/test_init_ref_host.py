"""CPU checks of the initialisation reference (``tests/_init_ref.py``): the exactness premises of the exact-arithmetic
inputs, the finish replica against the reference's fixtures and scikit-learn's own loop, the derived bounds of the
projection on NumPy's float64 in two feature orders (they are not vacuous on the host), the isolation of every discrete
decision in the whole-initialisation cases, and the separable replica against the fixture, with every round's lead.

Finding recorded here (``test_signatures_depend_on_the_bits_of_the_norms``): the NNDSVD signatures and the column recipe
depend on ``pos2`` / ``neg2`` not only through ``take_neg`` -- ``lbd = sqrt(S_j sqrt(pos2_j) |y_p|)`` scales row j before the
threshold and the normalisation, so two sets of norms that differ in their last bits give signatures that differ in theirs.
A bit-for-bit comparison of the signatures therefore has to hand the host recipe the norms the device returned (themselves
held to the long-double norms within the derived bound); run with ``-s`` for the measured ratios."""

import os

import numpy as np
import pytest

import _init_ref as R
from conftest import REF_FIX
from salamander_amd import initialization as init
from salamander_amd.device_init import nndsvd_signature_side

L = R.L
# The float64 replica's spread recorded in test_gpu_init_entrywise.py (SEP_SPREAD = 2.7e-16, measured 2.63e-16 with this
# repository's NumPy) goes through BLAS (R @ u): another BLAS build may order the sums otherwise, so the CPU measurement is
# held to twice the recorded value -- a few ulps of norms[0] either way -- and the device tolerance stays 16 x the recorded one.
SEP_SPREAD_LIMIT = 2 * 2.7e-16


# ------------------------------------------------------------------------------------------------------ (1) premises
@pytest.mark.parametrize("N,V", R.GRAM_SHAPES + [(R.MANY_TILES_N, 96)])
def test_gram_inputs_are_exact_in_any_order(N, V):
    Xi = R.count_matrix(N, V)
    G, total = R.gram_exact(Xi)
    assert Xi.min() >= 0 and Xi.max() <= 255 and int(G.max()) < 2**53 and total < 2**53
    assert np.array_equal(G.astype(np.float64).astype(np.int64), G) and np.array_equal(G, G.T)
    assert np.array_equal(Xi.astype(np.uint16).astype(np.int64), Xi)  # the uint16 upload carries the same values
    X = Xi.astype(np.float64)
    assert np.array_equal(X.T @ X, G.astype(np.float64)) and np.array_equal(X[::-1].T @ X[::-1], G.astype(np.float64))
    if N >= 3:
        assert not Xi[N // 2].any() and Xi[N - 1, V - 1] == 255 and Xi[N - 1].sum() == 255
    if N * V >= 500:
        assert 0.25 < (Xi == 0).mean() < 0.4
    assert R.MANY_TILES_N > 16 * 4 * 256  # more tiles than an MI355X's Gram launch has waves (256 workgroups of four)


@pytest.mark.parametrize("N,V,K", R.PROJECT_SHAPES + [(R.MANY_ROWS, 96, 3)])
def test_projection_inputs_are_exact_in_any_order(N, V, K):
    Xi = R.count_matrix(N, V)
    B, Bi = R.sixteenths(K, V)
    U, pos2, neg2, bits = R.project_exact(Xi, Bi)
    assert np.abs(Bi).max() <= 16 and np.array_equal(B * 16, Bi)
    assert bits <= 53, bits  # every partial sum of every chain and of every sum of squares is a float64
    assert np.abs(U).max() < 2**16 and np.array_equal(U * 16, np.rint(U * 16))
    assert np.array_equal(pos2 * 256, np.rint(pos2 * 256)) and max(pos2.max(), neg2.max()) * 256 < 2**53
    if K >= 3:
        assert not B[K // 2].any() and not U[:, K // 2].any()
        assert not B[K - 1, : 96 * ((V - 1) // 96)].any()
    X = Xi.astype(np.float64)
    for rev in (False, True):
        U64, p64, n64 = R.project_f64(X, B, rev)
        assert np.array_equal(U64, U) and np.array_equal(p64, pos2) and np.array_equal(n64, neg2)


@pytest.mark.parametrize("N,V,K", R.FLAT_SHAPES)
def test_flat_replica_is_the_host_initialisation(N, V, K):
    Xi = R.count_matrix(N, V)
    post = R.flat_post(K, Xi)
    want = R.flat_replica(Xi, post)
    assert np.array_equal(want[N // 2], np.full(K, R.EPSILON))  # the all-zero sample
    floor = want == R.EPSILON
    half = floor[:, post == post[1]] if K > 1 else floor[:, :0]
    assert floor[:, post == 1e-12].all() and (K < 2 or 0.2 < half.mean() < 0.8) and (K < 3 or not floor[:, 2].all())
    # the host path's own statement: init_flat + normalize_WH + clip
    S, E = init.initialize_mat(Xi.astype(np.float64), K, "flat")
    colsum = np.full((K, V), 1.0 / V).sum(axis=1)
    assert np.array_equal(E, R.flat_replica(Xi, colsum))
    assert R.chunk_starts(70) == [0, 35] and R.chunk_starts(130) == [0, 44, 88] and R.chunk_starts(64) == [0]


# ------------------------------------------------------------------------------------------------ the finish replica
def _exact_svd_init(X, K, method):
    """initialize_on_device on the host: exact SVD through the Gram matrix, the finish replica in float64"""
    X = np.asarray(X, dtype=np.float64)
    evals, evecs = np.linalg.eigh(X.T @ X)
    order = np.argsort(evals)[::-1][:K]
    evals, evecs = evals[order], evecs[:, order]
    B = (evecs / np.sqrt(evals)).T
    U, pos2, neg2 = R.project_f64(X, B)
    S_raw, scale, take_neg, fill = nndsvd_signature_side(evals, evecs, pos2, neg2, K, X.mean(), method)
    return S_raw, U, scale, take_neg, fill


@pytest.mark.parametrize("method", ["nndsvd", "nndsvda"])
def test_finish_replica_reproduces_the_reference_fixtures(method):
    d = os.path.join(REF_FIX, "initialization")
    data = np.load(f"{d}/data_mat.npy")
    S_raw, U, scale, take_neg, fill = _exact_svd_init(data, 2, method)
    colsum = S_raw.sum(axis=1)
    E = R.finish_replica(U, scale, take_neg, colsum, R.ZERO_BELOW, fill)
    assert np.allclose((S_raw / colsum[:, None]).clip(R.EPSILON), np.load(f"{d}/signatures_mat_{method}_seed1.npy"), rtol=1e-7, atol=0)
    assert np.allclose(E, np.load(f"{d}/exposures_mat_{method}_seed1.npy"), rtol=1e-7, atol=0)


@pytest.mark.parametrize("method", ["nndsvd", "nndsvda"])
def test_finish_replica_reproduces_sklearns_loop(method):
    """30 x 12 counts, K = 5: sklearn's randomized SVD works on 5 + 10 oversampled directions >= the rank, so it is exact to
    rounding and its NNDSVD loop (``_initialize_nmf``) is comparable entry by entry; post = 1, sklearn's zeros at the floor."""
    sknmf = pytest.importorskip("sklearn.decomposition._nmf")
    rng = np.random.default_rng(3)
    X = rng.poisson(rng.gamma(1.0, 20.0, size=(30, 12))).astype(np.float64)
    np.random.seed(1)
    W_sk, H_sk = sknmf._initialize_nmf(X, 5, init=method)
    S_raw, U, scale, take_neg, fill = _exact_svd_init(X, 5, method)
    E = R.finish_replica(U, scale, take_neg, np.ones(5), R.ZERO_BELOW, fill)
    assert np.allclose(S_raw, H_sk, rtol=1e-7, atol=1e-12)
    assert np.allclose(E, np.maximum(W_sk, R.EPSILON), rtol=1e-7, atol=1e-12)
    assert (W_sk == 0).any() or method == "nndsvda"


@pytest.mark.parametrize("V,K", R.FINISH_SHAPES)
def test_finish_probes_tell_the_kernels_rules_apart(V, K):
    """The probes hit ZERO_BELOW and EPSILON exactly and one ulp to either side, and every rule of the kernel matters on them:
    a replica with one rule changed gives another result."""
    X, B, scale, take_neg, post, perm = R.finish_case(V, K)
    assert np.array_equal(X.sum(axis=1), np.ones(V)) and np.array_equal(X.sum(axis=0), np.ones(V))
    U = B.T[perm]  # what init_project leaves: H[n, j] = B[j, perm[n]]
    assert np.array_equal(X.astype(np.float64) @ B.T, U)
    part = np.where(take_neg[None, :].astype(bool), np.maximum(-U, 0), np.maximum(U, 0)) * scale[None, :]
    pow2 = np.isin(scale, [0.125, 0.5, 1.0, 4.0])
    for j in range(K):
        if pow2[j] and j > 0:
            col = part[:, j]
            assert (col == R.ZERO_BELOW).any() and (col == np.nextafter(R.ZERO_BELOW, 0)).any() and (col == np.nextafter(R.ZERO_BELOW, 1)).any(), j
    hits = (part * post[None, :] == R.EPSILON) & (part >= R.ZERO_BELOW)
    assert hits.any()
    starts = [j for j in R.chunk_starts(K) if j > 0] + ([64] if K > 64 else [])
    for j in [0] + starts:
        assert take_neg[j] == 0 and (U[:, j] < -1.0).any()
    for fill in R.FINISH_FILLS:
        want = R.finish_replica(U, scale, take_neg, post, R.ZERO_BELOW, fill)
        assert want.min() >= R.EPSILON and np.isfinite(want).all()
        assert (want == R.EPSILON).any()
        # one rule changed at a time
        v = np.where(take_neg[None, :].astype(bool), np.where(U < 0, -U, 0.0), np.where(U > 0, U, 0.0)) * scale[None, :]
        v[:, 0] = np.abs(U[:, 0]) * scale[0]

        def rest(v, le=False, clip=True, fill_first=False):
            v = v.copy()
            if fill_first and fill:
                v[v == 0] = fill
            v[(v <= R.ZERO_BELOW) if le else (v < R.ZERO_BELOW)] = 0.0
            if fill and not fill_first:
                v[v == 0] = fill
            out = v * post[None, :]
            return np.where(out < R.EPSILON, R.EPSILON, out) if clip else out

        assert np.array_equal(rest(v), want)
        assert not np.array_equal(rest(v, le=True), want), "'<=' for '<' goes unseen"
        assert not np.array_equal(rest(v, clip=False), want), "a missing final clip goes unseen"
        if fill:
            assert not np.array_equal(rest(v, fill_first=True), want), "the fill before the threshold goes unseen"
        no_neg = R.finish_replica(U, scale, np.zeros(K, dtype=np.int32), post, R.ZERO_BELOW, fill)
        assert K == 1 or not np.array_equal(no_neg[:, 1], want[:, 1]), "take_neg ignored goes unseen"
        for j in starts:
            everywhere = R.finish_replica(U, scale, take_neg, post, R.ZERO_BELOW, fill, first_cols=(0, j))
            assert not np.array_equal(everywhere[:, j], want[:, j]), f"|x| in column {j} goes unseen"
    assert 2.0**-20 * post.min() < R.EPSILON < 0.25 * post.min()


# ------------------------------------------------------------------------------------------ (2) the derived bounds
def test_projection_bounds_hold_for_numpy_float64_in_two_feature_orders():
    worst_u, worst_n = (0.0, None), (0.0, None)
    for N, V, K in R.PROJECT_SHAPES:
        X, B = R.generic_case(N, V, K)
        U, a, p, n = R.project_ld(X, B)
        for rev in (False, True):
            ru, rn = R.project_ratios(*R.project_f64(X, B, rev), U, a, p, n, N, V)
            worst_u, worst_n = max(worst_u, (ru, (N, V, K))), max(worst_n, (rn, (N, V, K)))
            assert ru <= 1.0 and rn <= 1.0, (N, V, K, rev, ru, rn)
    print(f"\n[init-ref] NumPy float64 projection: worst entry {worst_u[0] * (worst_u[1][1] + 2):.2f} x 2^-53 a = {worst_u[0]:.4f} of its bound at {worst_u[1]}; "
          f"worst norm {worst_n[0]:.4f} of its bound at {worst_n[1]}")
    assert worst_u[0] > 0.0  # the bound is in the right unit: float64 is not exact here


# --------------------------------------------------------------------------------- (3) the whole initialisation cases
@pytest.mark.parametrize("V,N,K,method", R.WHOLE_CASES)
def test_every_discrete_decision_of_the_whole_cases_is_isolated(V, N, K, method):
    h = R.WholeHost(V, N, K, method)
    assert not h.X[N // 3].any() and np.array_equal(h.X[N - 2], h.X[1]) and (h.X == 0).mean() > 0.05
    r = h.recipe(h.pos2, h.neg2)
    iso = h.isolation(r)
    print(f"\n[init-ref] whole V={V} N={N} K={K} {method}: {iso}")
    assert iso["sign"] == 0 and iso["thresh"] == 0 and iso["zero"] == 0 and iso["floor"] == 0 and iso["finite"] and iso["min_eval"] > 1.0, iso
    # float64 in both feature orders makes the decisions the long-double side makes, and stays within the entry bound
    worst_n = worst_e = 0.0
    for rev in (False, True):
        U64, p64, n64 = R.project_f64(h.X, h.B, rev)
        worst_n = max(worst_n, float((np.maximum(np.abs(p64.astype(L) - h.pos2), np.abs(n64.astype(L) - h.neg2)) / h.bound_n).max()))
        r64 = h.recipe(p64, n64)
        assert np.array_equal(r64["take_neg"], r["take_neg"])
        E64 = R.finish_replica(U64, r64["scale"], r64["take_neg"], r64["post"], R.ZERO_BELOW, r64["fill"])
        E_own, exact_own, bound_own = h.exposures(r64)  # the long-double U under the recipe this float64 side used
        assert np.array_equal(E64[exact_own], E_own[exact_own].astype(np.float64))
        worst_e = max(worst_e, float((np.abs(E64.astype(L) - E_own)[~exact_own] / bound_own[~exact_own]).max()))
    print(f"[init-ref] whole V={V} N={N} K={K} {method}: NumPy float64 norms {worst_n:.4f} of their bound, exposures {worst_e:.4f} of (V + 4) 2^-53 a scale post")
    assert worst_n <= 1.0 and worst_e <= 1.0


def test_signatures_depend_on_the_bits_of_the_norms():
    """Two float64 projections of one case (ascending and descending feature order) make every decision alike, and their
    signatures still differ in the last bits: the norms enter through lbd, not only through take_neg."""
    V, N, K, method = R.WHOLE_CASES[0]
    h = R.WholeHost(V, N, K, method)
    (_, p0, n0), (_, p1, n1) = R.project_f64(h.X, h.B, False), R.project_f64(h.X, h.B, True)
    assert not (np.array_equal(p0, p1) and np.array_equal(n0, n1))
    r0, r1 = h.recipe(p0, n0), h.recipe(p1, n1)
    assert np.array_equal(r0["take_neg"], r1["take_neg"])
    assert not np.array_equal(r0["S"], r1["S"]) and np.allclose(r0["S"], r1["S"], rtol=1e-12, atol=0)
    r2 = h.recipe(p0.copy(), n0.copy())
    assert np.array_equal(r0["S"], r2["S"]) and np.array_equal(r0["scale"], r2["scale"])  # same norms, same bits


# --------------------------------------------------------------------------------------- (4) the separable selection
def test_separable_replica_gives_the_fixtures_indices():
    d = os.path.join(REF_FIX, "initialization")
    data = np.load(f"{d}/data_mat.npy")
    for dtype in (L, np.float64):
        chosen, norms, margins = R.separable_replica(data, 2, dtype)
        S = data[chosen].astype(float)
        S /= S.sum(axis=1, keepdims=True)
        assert np.allclose(S.clip(R.EPSILON), np.load(f"{d}/signatures_mat_separableNMF_seed1.npy"))
    assert margins.min() > 1e-9


@pytest.mark.parametrize("N,V,K", R.SEPARABLE_SHAPES)
def test_separable_rounds_are_isolated(N, V, K):
    X = R.separable_counts(N, V, K)
    (chosen, norms, margins), spread = R.separable_spread(X, K)
    print(f"\n[init-ref] separable N={N} V={V} K={K}: smallest lead {margins.min():.3g}, float64 spread {spread:.3g} of norms[0]")
    assert margins.min() > 1e-9 and len(set(chosen.tolist())) == K
    assert spread <= SEP_SPREAD_LIMIT
    assert np.array_equal(R.separable_replica(X, K, np.float64)[0], chosen)


def test_separable_rank3_catalogue_collapses_after_three_rounds():
    X = R.rank3_catalogue()
    (chosen, norms, margins), spread = R.separable_spread(X, 6)
    print(f"\n[init-ref] separable rank-3 catalogue: leads {margins[:3]}, float64 spread {spread:.3g}, later norms {np.asarray(norms[3:], dtype=float)}")
    assert margins[:3].min() > 1e-9 and (norms[3:] <= 1e-12 * norms[0]).all() and spread <= SEP_SPREAD_LIMIT
    for k in range(3):  # duplicates tie exactly: the lowest index of the winner's copies
        assert chosen[k] == np.flatnonzero((X == X[chosen[k]]).all(axis=1))[0]


@pytest.mark.parametrize("variant", sorted(R.TIE_ROWS))
def test_separable_tie_case_has_exact_ties_with_a_clear_lead(variant):
    X, want = R.tie_case(variant)
    ia, ib = R.TIE_ROWS[variant]
    for idx in (ia, ib):
        assert all(np.array_equal(X[i], X[idx[0]]) for i in idx)
    wg = lambda n: (n % 16384) // 16
    if variant == "spread":  # other workgroups, other slots, and two copies in one thread's two sweeps
        assert len({wg(i) for i in ia}) >= 3 and wg(3) == wg(10) and 3 % 16 != 10 % 16 and (wg(19), 19 % 16) == (wg(16403), 16403 % 16)
    elif variant == "last":
        assert wg(min(ia)) == 1023 and wg(max(ia)) == 0
    else:  # one selection thread reads both workgroups, the lower row in the later one
        for idx in (ia, ib):
            lo, hi = min(idx), max(idx)
            assert wg(hi) % 256 == wg(lo) % 256 and wg(hi) < wg(lo)
    (chosen, norms, margins), spread = R.separable_spread(X, 2)
    assert chosen.tolist() == want and margins.min() > 1e-9, (chosen, margins)
    assert R.separable_replica(X, 2, np.float64)[0].tolist() == want and spread <= SEP_SPREAD_LIMIT
