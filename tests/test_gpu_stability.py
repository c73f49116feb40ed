"""Signature stability on the device against the host replica (tests/_stability_ref.py): the stand-alone kernel, the form
that reads a batch's signatures in place, and KLNMFSweep(stability=True).

Assignments, round counts and the converged flag must be equal; that is a fair demand because every test asserts, from the
replica, that each assignment problem's optimum is isolated by a margin of 1e-6 -- no rounding can pick another one.
a, b and the consensus signatures agree to 4 (V + M + 8) 2^-52: a dot product of two vectors of norm <= 1 and <= M over V
terms carries at most about V 2^-53 M error in any summation order, the sums over M members add M 2^-53 M, and both are
divided by M or M - 1.  The silhouette (b - a) / max(a, b) and the scores built from it agree to 1e-9 once
max(a, b) >= 1e-6 has been asserted for every point, since that quotient is what conditions them."""

import numpy as np
import pytest

import salamander_amd as sal
import _stability_ref as ref
from salamander_amd.batch import BatchEngine

pytestmark = pytest.mark.gpu

FIELDS = ("assignments", "n_rounds", "converged", "consensus", "a", "b", "silhouette", "cluster_stability", "stability_mean", "stability_min")


def check(got, want, label=""):
    M, K = want.assignments.shape
    V = want.consensus.shape[1]
    tol = 4 * (V + M + 8) * 2.0**-52
    assert want.margins.min() > 1e-6, (label, want.margins.min())  # (a condition on the input, not on the kernel)
    print(f"{label}: K={K} M={M} V={V} rounds={want.n_rounds} margin={want.margins.min():.3g} "
          f"da={np.abs(got.a - want.a).max():.3g} db={np.nanmax(np.abs(got.b - want.b)) if K > 1 else 0:.3g} "
          f"dcons={np.abs(got.consensus - want.consensus).max():.3g} dsil={np.abs(got.silhouette - want.silhouette).max():.3g} tol={tol:.3g}")
    assert np.array_equal(got.assignments, want.assignments), label
    assert got.assignments.dtype == np.int32
    assert got.n_rounds == want.n_rounds and got.converged == want.converged, (label, got.n_rounds, want.n_rounds)
    assert np.abs(got.a - want.a).max() <= tol, label
    assert np.abs(got.consensus - want.consensus).max() <= tol, label
    assert np.allclose(got.consensus.sum(axis=1), 1.0, rtol=0, atol=1e-13)
    if K == 1:
        assert np.isnan(got.b).all() and np.array_equal(got.silhouette, np.ones((M, 1)))
    else:
        assert np.abs(got.b - want.b).max() <= tol, label
        assert np.maximum(want.a, want.b).min() >= 1e-6, label
    assert np.abs(got.silhouette - want.silhouette).max() <= 1e-9, label
    assert np.abs(got.cluster_stability - want.cluster_stability).max() <= 1e-9, label
    assert abs(got.stability_mean - want.stability_mean) <= 1e-9 and abs(got.stability_min - want.stability_min) <= 1e-9, label
    assert got.a.shape == got.b.shape == got.silhouette.shape == (M, K) and got.consensus.shape == (K, V)


def multi_round():
    """Eight signatures pulled half way to their mean, noise of coefficient of variation 1: the first round, matched
    against one noisy member, gets members wrong and the centroids correct them over several rounds."""
    return ref.planted(8, 24, 96, 1.0, 4, mix=0.5)[0]


@pytest.mark.parametrize("K,M,cv", [(5, 24, 0.05), (5, 24, 0.3), (8, 64, 0.05), (8, 64, 0.3), (16, 100, 0.05), (16, 100, 0.3)])
def test_planted_structure(K, M, cv):
    sigs, perms = ref.planted(K, M, 96, cv, seed=K + M)
    want = ref.stability(sigs)
    got = sal.signature_stability(sigs)
    check(got, want, f"planted cv={cv}")
    assert np.array_equal(got.assignments, ref.expected_assignments(perms, 0)) and got.n_rounds == 2 and got.converged


@pytest.mark.parametrize("V", [83, 96])
@pytest.mark.parametrize("K", [1, 2, 3, 15, 16])
@pytest.mark.parametrize("M", [2, 3, 17])
def test_shapes(K, M, V):
    sigs, _ = ref.planted(K, M, V, 0.3, seed=100 * K + M + V)
    check(sal.signature_stability(sigs), ref.stability(sigs), "shapes")


def test_anchor_is_the_member_of_smallest_error():
    sigs, perms = ref.planted(6, 9, 96, 0.3, seed=3)
    errors = np.array([5.0, 4.0, 3.0, 9.0, 1.0, 7.0, 1.0, 8.0, 2.0])  # member 4, the first of the two smallest
    want = ref.stability(sigs, errors)
    assert want.anchor == 4
    got = sal.signature_stability(sigs, errors)
    check(got, want, "anchor")
    assert np.array_equal(got.assignments, ref.expected_assignments(perms, 4))
    assert np.array_equal(got.assignments[4], np.arange(6))
    assert not np.array_equal(got.assignments, sal.signature_stability(sigs).assignments)


def test_two_groups_of_different_k_in_one_launch():
    a, _ = ref.planted(3, 17, 96, 0.3, seed=11)
    b, _ = ref.planted(16, 5, 96, 0.05, seed=12)
    ea, eb = np.arange(17, 0, -1.0), np.array([3.0, 1.0, 2.0, 5.0, 4.0])
    got = sal.signature_stability([a, b], [ea, eb])
    assert isinstance(got, list) and len(got) == 2
    check(got[0], ref.stability(a, ea), "group 0")
    check(got[1], ref.stability(b, eb), "group 1")
    alone = sal.signature_stability(b, eb)
    for f in FIELDS:
        assert np.array_equal(getattr(alone, f), getattr(got[1], f), equal_nan=True), f  # a group does not see its neighbours


def test_more_than_two_rounds_and_the_round_cap():
    sigs = multi_round()
    want = ref.stability(sigs)
    assert want.n_rounds > 2 and want.converged  # (6 rounds in the replica)
    check(sal.signature_stability(sigs), want, "multi-round")
    first = ref.stability(sigs, max_rounds=1)
    assert not np.array_equal(first.assignments, want.assignments)
    got = sal.signature_stability(sigs, max_rounds=1)
    assert got.n_rounds == 1 and not got.converged
    check(got, first, "max_rounds=1")
    capped = ref.stability(sigs, max_rounds=3)
    assert not capped.converged
    check(sal.signature_stability(sigs, max_rounds=3), capped, "max_rounds=3")


def test_same_call_twice_same_bits():
    sigs = multi_round()
    big, _ = ref.planted(16, 100, 96, 0.3, seed=5)
    for s in (sigs, big):
        r1, r2 = sal.signature_stability(s), sal.signature_stability(s)
        for f in FIELDS:
            assert np.array_equal(getattr(r1, f), getattr(r2, f), equal_nan=True), f


def test_refusals_before_any_launch():
    good, _ = ref.planted(4, 5, 96, 0.3, seed=1)
    with pytest.raises(ValueError, match="16"):
        sal.signature_stability(np.ones((3, 17, 96)))
    with pytest.raises(ValueError, match="96"):
        sal.signature_stability(np.ones((3, 4, 97)))
    with pytest.raises(ValueError, match="at least 2"):
        sal.signature_stability(good[:1])
    zero = good.copy()
    zero[2, 1] = 0.0
    with pytest.raises(ValueError, match="positive norm"):
        sal.signature_stability(zero)
    nan = good.copy()
    nan[3, 0, 7] = np.nan
    with pytest.raises(ValueError, match="finite"):
        sal.signature_stability(nan)
    with pytest.raises(ValueError):
        sal.signature_stability(good, max_rounds=0)
    # the C ABI refuses the same on its own (no launch: the message names the argument)
    import ctypes

    from salamander_amd import _lib
    from salamander_amd.stability import _Outputs

    lib = _lib.load()
    padded = np.zeros((5, 16, 96))
    padded[:, :4] = good
    padded[2, 1] = 0.0
    out = _Outputs([(5, 4)])
    ks, ms = (ctypes.c_int * 1)(4), (ctypes.c_int * 1)(5)
    assert lib.salnmf_signature_stability(0, padded.ctypes.data_as(_lib._D), 1, ks, ms, 96, None, 20, *out.pointers()) != 0
    assert "positive norm" in lib.salnmf_batch_last_error().decode()
    ms[0] = 1
    assert lib.salnmf_signature_stability(0, padded.ctypes.data_as(_lib._D), 1, ks, ms, 96, None, 20, *out.pointers()) != 0
    assert "at least 2" in lib.salnmf_batch_last_error().decode()
    # a batch group that mixes numbers of signatures, or is too small
    batch = BatchEngine(32, 96, [3, 3, 4])
    try:
        with pytest.raises(ValueError, match="share"):
            batch.stability([[0, 1, 2]])
        with pytest.raises(ValueError, match="at least 2"):
            batch.stability([[2]])
        with pytest.raises(ValueError):
            batch.stability([[0, 7]])
        offs, mem = (ctypes.c_int * 2)(0, 3), (ctypes.c_int * 3)(0, 1, 2)
        out = _Outputs([(3, 3)])
        assert lib.salnmf_batch_stability(batch._h, 1, offs, mem, None, 20, *out.pointers()) != 0
        assert "mixes" in lib.salnmf_batch_last_error().decode()
    finally:
        batch.close()


def planted_counts(seed=0, n_samples=160, n_signatures=4):
    rng = np.random.default_rng(seed)
    W = rng.dirichlet(np.full(96, 0.15), size=n_signatures)
    H = rng.gamma(1.0, 600.0, size=(n_samples, n_signatures))
    return rng.poisson(H @ W).astype(np.float64)


SWEEP = dict(ns_signatures=range(2, 6), seeds=range(2), n_resamples=3, init_method="random", min_iterations=200, max_iterations=200)


@pytest.fixture(scope="module")
def sweeps():
    X = planted_counts()
    with_stability = sal.models.KLNMFSweep(stability=True, **SWEEP)
    with_stability.fit(sal.AnnData(X.copy()))
    plain = sal.models.KLNMFSweep(**SWEEP)
    plain.fit(sal.AnnData(X.copy()))
    return with_stability, plain


def test_sweep_stability_equals_the_replica(sweeps):
    s, _ = sweeps
    ns = list(SWEEP["ns_signatures"])
    assert s.batched_.all() and "stability_s" in s.timings_
    assert s.stability_mean_.shape == s.stability_min_.shape == s.stability_rounds_.shape == s.stability_converged_.shape == (len(ns),)
    means, lows = [], []
    for g, K in enumerate(ns):
        members = s.models_[6 * g : 6 * g + 6]
        assert all(m.n_signatures == K for m in members)
        sigs = np.stack([np.asarray(m.asignatures.X) for m in members])
        want = ref.stability(sigs, [m.reconstruction_error for m in members])
        got = sal.stability.StabilityResult(
            s.assignments_[g], int(s.stability_rounds_[g]), bool(s.stability_converged_[g]), s.consensus_signatures_[g],
            want.a, want.b, s.silhouettes_[g], s.cluster_stability_[g], float(s.stability_mean_[g]), float(s.stability_min_[g]))
        # (the sweep keeps no a / b of its own: those two are checked on the same members in the in-place test below)
        check(got, want, f"sweep K={K}")
        means.append(want.stability_mean)
        lows.append(want.stability_min)
    assert s.suggest_n_signatures() == ref.suggest(ns, means, lows)
    assert s.suggest_n_signatures(0.0, -1.0) == 5 and s.suggest_n_signatures(1.5, 0.2) is None


def test_sweep_fits_do_not_change_with_stability(sweeps):
    s, plain = sweeps
    assert "stability_s" not in plain.timings_ and np.isnan(plain.stability_mean_).all()
    assert np.array_equal(s.reconstruction_errors_, plain.reconstruction_errors_)
    assert np.array_equal(s.resamples_, plain.resamples_)
    for a, b in zip(s.models_, plain.models_):
        assert np.array_equal(a.asignatures.X, b.asignatures.X)
        assert np.array_equal(a.adata.obsm["exposures"], b.adata.obsm["exposures"])
        assert a.history["objective_function"] == b.history["objective_function"] and a.n_iterations_ == b.n_iterations_


def test_in_place_equals_stand_alone_bit_for_bit():
    X = planted_counts(seed=1, n_samples=64)
    Ks = [3, 3, 3, 5, 5, 5, 5]
    rng = np.random.default_rng(2)
    batch = BatchEngine(64, 96, Ks)
    try:
        batch.upload_X(X, clip=True)
        for m, K in enumerate(Ks):
            batch.upload_member(m, rng.dirichlet(np.ones(96), size=K), rng.gamma(1.0, 100.0, size=(64, K)))
        batch.kl_step(150, list(range(len(Ks))), [0] * len(Ks))
        errors = [list(batch.samplewise_kl()[:3].sum(axis=1)), list(batch.samplewise_kl()[3:].sum(axis=1))]
        groups = [[0, 1, 2], [6, 3, 5, 4]]  # (any order of members)
        errors[1] = [errors[1][i - 3] for i in groups[1]]
        in_place = batch.stability(groups, errors)
        W = [batch.download_member(m)[0] for m in range(len(Ks))]
    finally:
        batch.close()
    alone = sal.signature_stability([np.stack([W[m] for m in g]) for g in groups], errors)
    for g in range(2):
        check(in_place[g], ref.stability(np.stack([W[m] for m in groups[g]]), errors[g]), f"in place, group {g}")
        for f in FIELDS:
            assert np.array_equal(getattr(in_place[g], f), getattr(alone[g], f), equal_nan=True), (g, f)


# ------------------------------------------------------------------ the assignment solve on constructed cost tiles
# (tests/_stability_ref.py: block_group and the families on it; their properties are asserted in
# tests/test_stability_solver_host.py)
def same_bits(x, y, label=""):
    for f in FIELDS:
        assert np.array_equal(getattr(x, f), getattr(y, f), equal_nan=True), (label, f)


@pytest.mark.parametrize("V", ref.HARD_VS)
@pytest.mark.parametrize("K", ref.HARD_KS)
@pytest.mark.parametrize("family", list(ref.HARD_FAMILIES))
def test_hard_assignment_tiles(family, K, V):
    """One anchor of block indicators and one member whose first-round cost tile is prescribed: Machol-Wien costs and the
    chain tile (augmenting paths through all K columns), and a pair of optima 1e-6 .. 1e-4 apart."""
    sigs, errors, want = ref.hard_case(family, K, V)
    assert not ref.greedy_is_optimal(ref.first_tile(want))  # (a condition on the input: row minima do not solve it)
    check(sal.signature_stability(np.array(sigs), np.array(errors)), want, f"{family} V={V}")


@pytest.mark.parametrize("K,M", ref.DENSE_CASES)
def test_random_dense_tiles_over_many_rounds(K, M):
    sigs, errors, want = ref.hard_case("dense", K, M)
    assert want.converged and want.n_rounds > 4
    check(sal.signature_stability(np.array(sigs), np.array(errors), max_rounds=ref.DENSE_MAX_ROUNDS), want, "dense")


def hard_groups():
    cases = [ref.hard_case(f, K, 96) for f in ref.HARD_FAMILIES for K in (16, 15, 3)] + [ref.hard_case("dense", 16, 17), ref.hard_case("dense", 5, 65)]
    return [np.array(c[0]) for c in cases], [np.array(c[1]) for c in cases], [c[2] for c in cases]


def test_hard_groups_in_one_launch_equal_each_alone():
    sigs, errors, _ = hard_groups()
    together = sal.signature_stability(sigs, errors, max_rounds=ref.DENSE_MAX_ROUNDS)
    for g, (s, e) in enumerate(zip(sigs, errors)):
        same_bits(together[g], sal.signature_stability(s, e, max_rounds=ref.DENSE_MAX_ROUNDS), g)


@pytest.mark.parametrize("K", ref.HARD_KS)
def test_exact_tie_returns_one_of_the_optima(K):
    """Two member rows of the same bits: each optimum has a twin of equal cost, and the host and the device round the tile
    differently, so either may come back.  The twins give the same cluster sums, so the replica's last centroids price
    the device's assignment."""
    sigs, errors = ref.block_group([ref.exact_tie(K)], 96)
    want = ref.stability(sigs, errors)
    assert want.margins[1] == 0.0
    got = sal.signature_stability(sigs, errors)
    tol = 4 * (96 + 2 + 8) * 2.0**-52
    for m in range(2):
        assert sorted(got.assignments[m]) == list(range(K))
        D = 1.0 - want.centroids @ want.unit[m].T
        cost, best = D[np.arange(K), got.assignments[m]].sum(), D[np.arange(K), want.assignments[m]].sum()
        print(f"exact tie K={K} member {m}: cost - optimum = {cost - best:.3g}, K tol = {K * tol:.3g}")
        assert cost - best <= K * tol
    assert 2 <= got.n_rounds <= 20 and (got.converged or got.n_rounds == 20)
    same_bits(got, sal.signature_stability(sigs, errors))


@pytest.mark.parametrize("V", ref.HARD_VS)
def test_hard_members_in_place_equal_stand_alone_bit_for_bit(V):
    cases = [ref.hard_case(f, K, V) for f in ref.HARD_FAMILIES for K in (16, 3)]
    if V == 96:
        cases.append(ref.hard_case("dense", 16, 17))
    sigs, errors = [np.array(c[0]) for c in cases], [np.array(c[1]) for c in cases]
    Ks = [s.shape[1] for s in sigs for _ in s]
    rng = np.random.default_rng(6)
    batch = BatchEngine(16, V, Ks)
    try:
        groups, m = [], 0
        for s in sigs:
            groups.append(list(range(m, m + len(s))))
            for W in s:
                batch.upload_member(m, W, rng.gamma(1.0, 100.0, size=(16, W.shape[0])))
                m += 1
        in_place = batch.stability(groups, errors, max_rounds=ref.DENSE_MAX_ROUNDS)
    finally:
        batch.close()
    alone = sal.signature_stability(sigs, errors, max_rounds=ref.DENSE_MAX_ROUNDS)
    for g, c in enumerate(cases):
        check(in_place[g], c[2], f"hard, in place, group {g}")
        same_bits(in_place[g], alone[g], g)


@pytest.mark.parametrize("member", [0, 4])
@pytest.mark.parametrize("kind", ["nan", "zero"])
def test_a_signature_that_is_not_finite_in_place(kind, member):
    """Only the in-place form can see one (a fit that failed): the stand-alone entry refuses it.  The kernel forms no
    address from a cost: the solve's indices come from lane numbers and matched rows alone, and its result reaches memory
    through the permutation, which the hand-off completes.  So the call returns, the group's assignments are permutations,
    its minimum stability is NaN, and the healthy group of the same launch does not notice."""
    K, M = 5, 6
    healthy, _ = ref.planted(K, M, 96, 0.3, seed=21)
    bad, _ = ref.planted(K, M, 96, 0.3, seed=22)
    if kind == "nan":
        bad[member, 2, 7] = np.nan  # (member 0 is the anchor: errors all zero)
    else:
        bad[member, 2] = 0.0
    batch = BatchEngine(16, 96, [K] * (2 * M))
    try:
        for m, W in enumerate(np.concatenate([healthy, bad])):
            batch.upload_member(m, W, np.ones((16, K)))
        got = batch.stability([list(range(M)), list(range(M, 2 * M))])
    finally:
        batch.close()
    assert got[1].assignments.shape == (M, K) and all(sorted(p) == list(range(K)) for p in got[1].assignments)
    assert np.isnan(got[1].stability_min) and np.isnan(got[1].stability_mean)
    assert 1 <= got[1].n_rounds <= 20 and (got[1].converged or got[1].n_rounds == 20)
    check(got[0], ref.stability(healthy), "healthy neighbour")
    same_bits(got[0], sal.signature_stability(healthy))
    want = ref.lane_stability(bad)
    print(f"{kind} in member {member}: rounds {got[1].n_rounds} (lane replica {want.n_rounds}), NaN clusters {int(np.isnan(got[1].cluster_stability).sum())} ({int(np.isnan(want.cluster_stability).sum())})")
