"""The assignment solve of the stability kernel on the CPU: ``lane_assign`` (tests/_stability_ref.py), the lane-by-lane
restatement of ``stab_assign`` in csrc/salnmf_stability.h, against SciPy's ``linear_sum_assignment`` on random tiles, on
tiles whose augmenting paths are as long as they can be and on tiles that are not finite; and the measured properties of the
constructed groups that tests/test_gpu_stability.py runs on the device, so that no change to a generator makes a device case
vacuous."""

import numpy as np
import pytest

import _stability_ref as ref


def permutation(p, K):
    return sorted(int(x) for x in p) == list(range(K))


# ------------------------------------------------------------------ the lane solve against an exact one
@pytest.mark.parametrize("kind", ["uniform", "exponential", "integer"])
def test_lane_assign_equals_scipy_on_random_tiles(kind):
    """420 tiles per K = 1 .. 16 and distribution: 20 160 in all.  Where the lane solve returns another permutation than
    SciPy, the margin must be 0 (it never is for the continuous draws) and the two costs equal, which is exact for the
    integer costs 0 .. 3, where ties abound."""
    rng = np.random.default_rng({"uniform": 1, "exponential": 2, "integer": 3}[kind])
    n_tied = 0
    for K in range(1, 17):
        shape = (420, K, K)
        D = {"uniform": rng.random, "exponential": rng.standard_exponential}[kind](shape) if kind != "integer" else rng.integers(0, 4, shape).astype(float)
        pcol = ref.lane_assign(D, K)
        assert ((pcol[:, :K] >= 0) & (pcol[:, :K] < K)).all() and (pcol[:, K:] == -1).all()
        for d, pc in zip(D, pcol):
            got = ref.lane_permutation(pc, K)
            assert permutation(got, K) and np.array_equal(pc[got], np.arange(K))  # (the hand-off inverts pcol, nothing more)
            want, _ = ref.assign(d, margin=False)
            if not np.array_equal(got, want):
                n_tied += 1
                assert ref.assign(d)[1] == 0.0, (K, kind)
                assert d[np.arange(K), got].sum() == d[np.arange(K), want].sum(), (K, kind)
    print(f"{kind}: {n_tied} tiles with another optimum of the same cost")
    assert (n_tied > 1000) == (kind == "integer")  # (the tie rule is reached, and only where there are ties)


@pytest.mark.parametrize("K", range(2, 17))
def test_chain_tiles_need_every_column_for_every_row(K):
    """Row r's augmenting path and its tree pass through all r + 1 columns: the trip counts ``it <= r`` are needed in full."""
    D = ref.chain_tile(K)
    p, path, tree = ref.augmenting_paths(D)
    assert np.array_equal(path, np.arange(1, K + 1)) and np.array_equal(tree, path)
    assert np.array_equal(p, np.arange(K)[::-1]) and np.array_equal(p, ref.assign(D)[0]) and ref.assign(D)[1] > 1e-4
    assert np.array_equal(ref.lane_permutation(ref.lane_assign(D, K), K), p)
    E = D[:, np.random.default_rng(K).permutation(K)]  # columns in any order: the paths are as long, the lanes they cross differ
    assert ref.augmenting_paths(E)[1].max() == K
    assert np.array_equal(ref.lane_permutation(ref.lane_assign(E, K), K), ref.assign(E)[0])


def test_augmenting_paths_is_an_exact_solver():
    rng = np.random.default_rng(5)
    for K in range(1, 17):
        for D in rng.random((20, K, K)):
            p, path, tree = ref.augmenting_paths(D)
            assert np.array_equal(p, ref.assign(D, margin=False)[0])
            assert (path >= 1).all() and (path <= tree).all() and (tree <= np.arange(1, K + 1)).all()


# ------------------------------------------------------------------ tiles that are not finite
def non_finite_tiles(K, rng):
    base = rng.random((K, K))
    out = []
    for bad in (np.nan, np.inf):
        row, colm, both, one = base.copy(), base.copy(), base.copy(), base.copy()
        row[rng.integers(K)] = bad
        colm[:, rng.integers(K)] = bad
        both[rng.integers(K)] = bad
        both[:, rng.integers(K)] = bad
        one[rng.integers(K), rng.integers(K)] = bad
        out += [row, colm, both, one, np.full((K, K), bad)]
    out.append(np.where(rng.random((K, K)) < 0.3, np.nan, base))
    out.append(np.where(rng.random((K, K)) < 0.3, np.inf, base))
    out.append(np.full((K, K), -np.inf))
    return np.stack(out)


@pytest.mark.parametrize("K", range(1, 17))
def test_non_finite_tiles_end_and_stay_in_range(K):
    """The trip counts are fixed, so the solve ends; every lane's index is -1 or in [0, K), and the kernel's hand-off makes
    a permutation of whatever comes back."""
    rng = np.random.default_rng(100 + K)
    for _ in range(8):
        tiles = non_finite_tiles(K, rng)
        pcol = ref.lane_assign(tiles, K)
        assert pcol.shape == (len(tiles), 16) and ((pcol >= -1) & (pcol < K)).all()
        for pc in pcol:
            assert permutation(ref.lane_permutation(pc, K), K)
    for pc in (np.full(16, -1), np.zeros(16, dtype=int), np.full(16, K - 1), np.arange(16) % K):  # whatever comes back
        assert permutation(ref.lane_permutation(pc, K), K)


def test_a_single_infinite_entry_is_avoided():
    rng = np.random.default_rng(9)
    for K in range(2, 17):
        D = rng.random((K, K))
        D[rng.integers(K), rng.integers(K)] = np.inf
        assert np.array_equal(ref.lane_permutation(ref.lane_assign(D, K), K), ref.assign(D, margin=False)[0])


@pytest.mark.parametrize("kind", ["nan", "zero"])
def test_lane_stability_reports_a_row_that_is_not_finite(kind):
    """What the in-place form gets when a fit has failed: the kernel restated with the lane solve gives permutations, and
    the minimum cluster stability is NaN wherever the NaN cluster stands among the K."""
    for K, M, seed in ((5, 6, 1), (16, 9, 2), (3, 4, 3), (2, 3, 4)):
        for member in (0, M - 1):  # the anchor, another member
            sigs, _ = ref.planted(K, M, 96, 0.3, seed)
            if kind == "nan":
                sigs[member, K // 2, 7] = np.nan
            else:
                sigs[member, K // 2] = 0.0
            r = ref.lane_stability(sigs)
            assert all(permutation(p, K) for p in r.assignments)
            assert np.isnan(r.stability_min) and np.isnan(r.stability_mean) and np.isnan(r.cluster_stability).any()


# ------------------------------------------------------------------ the constructed groups of the device tests
def test_block_group_solves_the_prescribed_tile():
    rng = np.random.default_rng(0)
    for K, V in ((16, 96), (16, 83), (5, 96), (15, 83), (2, 83)):
        A = rng.random((K, K))
        for equal in (False, True):
            if equal:
                A = 0.5 + 0.5 * A
            sigs, errors = ref.block_group([A, A[::-1]], V, equal_norms=equal)
            assert sigs.shape == (3, K, V) and (sigs >= 0).all() and np.argmin(errors) == 0
            norm = np.sqrt((A * A).sum(axis=1))
            want = 1.0 - (A / (norm.max() if equal else norm[:, None])).T
            got = ref.first_tile(ref.stability(sigs, errors, max_rounds=1, margins=False))
            assert np.abs(got - want).max() <= 1e-15
    with pytest.raises(AssertionError):
        ref.block_group([np.diag(np.arange(1.0, 17.0)) + 1e-3], 83, equal_norms=True)  # (norms 1 : 16, blocks of 5)


# (family, K) -> the longest augmenting path, in columns, of the first round's tile: measured, and asserted as measured
LONGEST_PATH = {("machol_wien", 2): 2, ("machol_wien", 3): 3, ("machol_wien", 8): 8, ("machol_wien", 15): 15, ("machol_wien", 16): 16,
                ("long_path", 2): 2, ("long_path", 3): 3, ("long_path", 8): 8, ("long_path", 15): 15, ("long_path", 16): 16,
                ("near_tie", 2): 1, ("near_tie", 3): 1, ("near_tie", 8): 2, ("near_tie", 15): 4, ("near_tie", 16): 5}


@pytest.mark.parametrize("V", ref.HARD_VS)
@pytest.mark.parametrize("K", ref.HARD_KS)
@pytest.mark.parametrize("family", list(ref.HARD_FAMILIES))
def test_hard_pairs_meet_the_conditions_of_the_device_test(family, K, V):
    sigs, errors, want = ref.hard_case(family, K, V)
    assert sigs.shape == (2, K, V) and (sigs >= 0).all() and want.anchor == 0
    D = ref.first_tile(want)
    p, path, tree = ref.augmenting_paths(D)
    margin = want.margins.min()
    print(f"{family} K={K} V={V}: rounds {want.n_rounds}, longest path {path.max()}, largest tree {tree.max()}, margin {margin:.3g}, "
          f"smallest max(a, b) {np.maximum(want.a, want.b).min():.3g}")
    assert np.array_equal(p, want.assignments[1]) or want.n_rounds > 2
    assert path.max() == LONGEST_PATH[family, K]
    assert not ref.greedy_is_optimal(D)
    assert margin > 1e-6 and np.maximum(want.a, want.b).min() >= 0.11  # check()'s preconditions, with room
    if family == "near_tie":
        assert 1e-6 <= margin <= 1e-4
    if family == "long_path":
        assert np.array_equal(tree, np.arange(1, K + 1))
    # the kernel restated with the lane solve passes the device test's demands on these inputs
    lanes = ref.lane_stability(sigs, errors)
    assert np.array_equal(lanes.assignments, want.assignments) and (lanes.n_rounds, lanes.converged) == (want.n_rounds, want.converged)
    assert np.abs(lanes.silhouette - want.silhouette).max() <= 1e-9


def test_machol_wien_without_equal_norms_stops_at_nine_columns():
    """Why ``block_group`` has ``equal_norms``: dividing row i of A by its own norm moves the optimum.  The paths of the
    Machol-Wien tile shrink to 9 of 16 columns, and at K = 2 every row's own minimum becomes the optimum."""
    longest = {}
    for K in (2, 3, 15, 16):
        sigs, errors = ref.block_group([ref.machol_wien(K, 0)], 96)
        D = ref.first_tile(ref.stability(sigs, errors, max_rounds=1, margins=False))
        longest[K] = ref.augmenting_paths(D)[1].max()
        assert ref.greedy_is_optimal(D) == (K == 2)
    assert longest == {2: 1, 3: 2, 15: 9, 16: 9}


# (K, M) -> rounds of the replica, all converged
DENSE_ROUNDS = {(5, 65): 5, (16, 65): 16, (16, 17): 9}


@pytest.mark.parametrize("K,M", ref.DENSE_CASES)
def test_random_dense_groups_take_many_rounds(K, M):
    sigs, errors, want = ref.hard_case("dense", K, M)
    share = np.mean([ref.greedy_is_optimal(ref.first_tile(want, m)) for m in range(1, M)])
    print(f"dense K={K} M={M}: rounds {want.n_rounds}, margin {want.margins.min():.3g}, smallest max(a, b) {np.maximum(want.a, want.b).min():.3g}, "
          f"share of first-round tiles whose greedy assignment is optimal {share:.2f}")
    assert sigs.shape == (M, K, 96) and want.anchor == 0
    assert want.converged and want.n_rounds == DENSE_ROUNDS[K, M] and want.n_rounds > 4
    assert want.margins.min() > 1e-6 and np.maximum(want.a, want.b).min() >= 0.1
    assert share == 0.0 if K == 16 else 0.0 < share < 0.3
    lanes = ref.lane_stability(sigs, errors, ref.DENSE_MAX_ROUNDS)
    assert np.array_equal(lanes.assignments, want.assignments) and (lanes.n_rounds, lanes.converged) == (want.n_rounds, want.converged)


@pytest.mark.parametrize("K", ref.HARD_KS)
def test_exact_tie_has_margin_zero(K):
    sigs, errors = ref.block_group([ref.exact_tie(K)], 96)
    assert np.array_equal(sigs[1, 0], sigs[1, 1])
    want = ref.stability(sigs, errors)
    assert want.margins[1] == 0.0 and want.converged
    lanes = ref.lane_stability(sigs, errors)
    assert all(permutation(p, K) for p in lanes.assignments) and lanes.converged
    D = 1.0 - want.centroids @ want.unit[1].T
    cost = lambda p: D[np.arange(K), p].sum()
    assert abs(cost(lanes.assignments[1]) - cost(want.assignments[1])) <= K * 4 * (96 + 2 + 8) * 2.0**-52
