"""``sal.nb_assign_signatures`` and ``sal.estimate_dispersion(candidates=)`` on the device against the host
replica (tests/_nb_assign_ref.py), ``sal.nb_refit_exposures`` and themselves.

Decisions are compared exactly on the rows that the three host replicas leave isolated (tests/test_nb_assign_host.py shows the
share per case on the CPU); values within MARGIN = 16 x the host spreads recorded in tests/_nb_assign_ref.py, which were
measured on the CPU on these inputs.  No tolerance is tuned on the device; every figure is printed before it is asserted."""

import functools

import numpy as np
import pytest

import _assign_masks_ref as amr
import _nb_assign_ref as nar
import _nb_ref as nref
import salamander_amd as sal
from salamander_amd import _lib

pytestmark = pytest.mark.gpu

H_TOL = nar.MARGIN * nar.H_SPREAD
F_TOL = nar.MARGIN * nar.F_SPREAD
FIXED = nar.FIXED
IDS = [f"P{c[0]}-K{c[1]}-V{c[2]}-{c[4]}" for c in nar.CASES]
FIELDS = ("exposures", "active", "reconstruction_errors", "removal_round", "kl_increase", "n_trials", "n_iterations", "converged", "dense_exposures",
          "dense_errors", "dense_n_iterations", "dense_converged", "readd_round", "kl_decrease")


def same(a, b, rows_a=slice(None), rows_b=slice(None)):
    for name in FIELDS:
        x, y = getattr(a, name), getattr(b, name)
        assert (x is None) == (y is None), name
        if x is not None:
            assert np.array_equal(x[rows_a], y[rows_b], equal_nan=True), name


@functools.lru_cache(maxsize=None)
def device_case(*case):
    X, W, alpha, kw, _, _ = nar.case_replicas(*case)
    return sal.nb_assign_signatures(X, W, alpha, **FIXED, **kw)


@pytest.mark.parametrize("case", nar.CASES, ids=IDS)
def test_decisions_and_values_against_the_replica(case):
    X, W, alpha, kw, runs, (ok, _, _) = nar.case_replicas(*case)
    ld = runs[2]
    got = device_case(*case)
    rows = np.flatnonzero(ok)
    C, R = ld.candidates, ld.required
    assert np.array_equal(got.active[rows], ld.active[rows])
    assert np.array_equal(got.removal_round[rows], ld.removal_round[rows])
    if kw["readd"]:
        assert np.array_equal(got.readd_round[rows], ld.readd_round[rows])
        assert np.array_equal(np.isnan(got.kl_decrease[rows]), np.isnan(ld.kl_decrease[rows].astype(np.float64)))
    assert np.array_equal(got.n_trials[rows], ld.n_trials[rows]) and np.array_equal(got.n_iterations[rows], ld.n_iterations[rows])
    assert np.array_equal(np.isnan(got.kl_increase[rows]), np.isnan(ld.kl_increase[rows].astype(np.float64)))
    assert np.array_equal(got.n_iterations, 20 * (got.n_trials.astype(np.int64) + 1))
    assert (got.exposures[~C] == 0.0).all() and not got.active[~C].any() and np.isnan(got.kl_increase[~C]).all()
    assert (got.removal_round[~C] == -1).all()
    if kw["readd"]:
        assert np.isnan(got.kl_decrease[~C]).all() and (got.readd_round[~C] == -1).all()
    assert np.array_equal(got.exposures == 0.0, ~got.active)
    assert got.active[R].all() and np.isnan(got.kl_increase[R]).all()
    scale = nar.row_scale(X, W, alpha, ld.exposures)
    dH, dF = amr.deviations(got, ld, scale, rows)
    print(f"{case}: {rows.size} of {ok.size} rows isolated; H device {dH:.3g} tol {H_TOL:.3g}; f device {dF:.3g} tol {F_TOL:.3g}")
    assert dH <= H_TOL and dF <= F_TOL
    assert np.array_equal(got.log_likelihood, -got.reconstruction_errors + nref.constant(X, alpha))
    assert np.array_equal(got.dense_log_likelihood, -got.dense_errors + nref.constant(X, alpha))
    assert np.array_equal(got.dispersion, alpha)


def same_dense(got, fit, rows=slice(None)):
    assert np.array_equal(got.dense_exposures[rows], fit.exposures)
    assert np.array_equal(got.dense_errors[rows], fit.reconstruction_errors)
    assert np.array_equal(got.dense_n_iterations[rows], fit.n_iterations)
    assert np.array_equal(got.dense_converged[rows], fit.converged)


CONVERGING = dict(min_iterations=30, max_iterations=200, conv_test_freq=10, tol=1e-5)


@pytest.mark.parametrize("K,solve", [(3, FIXED), (17, FIXED), (64, FIXED), (96, FIXED), (17, CONVERGING)], ids=["K3", "K17", "K64", "K96", "K17-converging"])
def test_phase_0_is_the_dense_refit_bit_for_bit(K, solve):
    X, W = nref.catalogue(17, K, 96, seed=K)
    alpha = nref.mixed_alpha(17)
    same_dense(sal.nb_assign_signatures(X, W, alpha, **solve), sal.nb_refit_exposures(X, W, alpha, **solve))


def sub_call(X, W, alpha, C, rows, **kw):
    idx = np.flatnonzero(C)
    return idx, sal.nb_assign_signatures(X[rows], W[idx], alpha[rows], **FIXED, **kw)


@pytest.mark.parametrize("case", [c for c in nar.CASES if c[4] in ("prefix", "word") or (c[4] == "shared" and c[1] == 16)],
                         ids=lambda c: f"K{c[1]}-{c[4]}")
def test_sets_against_the_sub_catalogue(case):
    """Phase 0 against nb_refit_exposures and the whole call against the call on W[C], for shared sets: bit for bit where the
    sub-catalogue has the same KT and keeps every signature's position (`prefix`), decisions and the value bound otherwise."""
    X, W, alpha, kw, _, (ok, _, _) = nar.case_replicas(*case)
    got = device_case(*case)
    C = np.broadcast_to(kw["candidates"], (X.shape[0], W.shape[0]))[0]
    idx, sub = sub_call(X, W, alpha, C, slice(None), max_kl_increase=kw["max_kl_increase"], readd=kw["readd"])
    fit = sal.nb_refit_exposures(X, W[idx], alpha, **FIXED)
    assert (got.dense_exposures[:, ~C] == 0.0).all()
    if case[4] == "prefix":
        same_dense(type("R", (), dict(dense_exposures=got.dense_exposures[:, idx], dense_errors=got.dense_errors,
                                      dense_n_iterations=got.dense_n_iterations, dense_converged=got.dense_converged)), fit)
        for name in FIELDS:
            x, y = getattr(got, name), getattr(sub, name)
            if x is not None:
                assert np.array_equal(x[:, idx] if x.ndim == 2 else x, y, equal_nan=True), name
        return
    rows = np.flatnonzero(ok)
    dH0 = float((np.abs(got.dense_exposures[:, idx] - fit.exposures) / np.maximum(fit.exposures, nar.EPSILON)).max())
    scale = nar.row_scale(X, W, alpha, got.dense_exposures)
    dF0 = float((np.abs(got.dense_errors - fit.reconstruction_errors) / scale).max())
    assert np.array_equal(got.active[rows][:, idx], sub.active[rows]) and np.array_equal(got.removal_round[rows][:, idx], sub.removal_round[rows])
    assert np.array_equal(got.n_trials[rows], sub.n_trials[rows])
    wide = type("R", (), {n: (getattr(got, n)[:, idx] if getattr(got, n) is not None and getattr(got, n).ndim == 2 else getattr(got, n)) for n in FIELDS})
    dH, dF = amr.deviations(wide, type("R", (), {n: getattr(sub, n) for n in FIELDS}), scale, rows)
    print(f"{case}: phase 0 H {dH0:.3g} f {dF0:.3g}; whole call H {dH:.3g} f {dF:.3g}; tol {H_TOL:.3g} {F_TOL:.3g}")
    assert max(dH0, dH) <= H_TOL and max(dF0, dF) <= F_TOL


def test_an_active_set_solve_is_reachable():
    X, W = nref.catalogue(17, 33, 96, seed=2)
    alpha = nref.mixed_alpha(17)
    A, _ = amr.case_sets(17, 33, 2, "random")
    got = sal.nb_assign_signatures(X, W, alpha, candidates=A, required=A, **FIXED)
    assert not got.n_trials.any() and np.array_equal(got.exposures, got.dense_exposures) and np.array_equal(got.active, A)
    assert np.array_equal(got.exposures == 0.0, ~A) and np.array_equal(got.n_iterations, np.full(17, 20))
    again = sal.nb_assign_signatures(X, W, alpha, candidates=A, required=A, readd=True, **FIXED)
    assert np.array_equal(again.exposures, got.exposures) and not again.n_trials.any()
    assert (again.readd_round == -1).all() and np.isnan(again.kl_decrease).all()
    # required covering all candidates: nothing to remove, nothing left to re-add
    every = sal.nb_assign_signatures(X, W, alpha, required=np.ones(33, dtype=bool), readd=True, **FIXED)
    assert not every.n_trials.any() and every.active.all() and np.array_equal(every.exposures, every.dense_exposures)


@functools.lru_cache(maxsize=None)
def independence_inputs():
    P, K = 40, 17
    X, W = nref.catalogue(P, K, 96, seed=11)
    C, R = amr.case_sets(P, K, 11, "required")
    kw = dict(max_kl_increase=0.5, readd=True, **FIXED)
    alpha = nref.mixed_alpha(P)
    return X, W, alpha, C, R, kw, sal.nb_assign_signatures(X, W, alpha, candidates=C, required=R, **kw)


@pytest.mark.parametrize("N", [1, 15, 16, 17])
def test_a_row_subset_equals_the_full_call(N):
    X, W, alpha, C, R, kw, full = independence_inputs()
    rows = np.arange(40)[-N:]
    same(sal.nb_assign_signatures(X[rows], W, alpha[rows], candidates=C[rows], required=R[rows], **kw), full, rows_b=rows)


def test_rows_permuted_scalar_dispersion_and_nan_surroundings():
    X, W, alpha, C, R, kw, full = independence_inputs()
    perm = np.random.default_rng(3).permutation(40)
    same(sal.nb_assign_signatures(X[perm], W, alpha[perm], candidates=C[perm], required=R[perm], **kw), full, rows_b=perm)
    same(sal.nb_assign_signatures(X, W, 20.0, candidates=C, required=R, **kw),
         sal.nb_assign_signatures(X, W, np.full(40, 20.0), candidates=C, required=R, **kw))
    big_X, big_W, big_a = np.full((42, 98), np.nan), np.full((19, 98), np.nan), np.full(42, np.nan)
    big_X[1:41, 1:97], big_W[1:18, 1:97], big_a[1:41] = X, W, alpha
    same(sal.nb_assign_signatures(big_X[1:41, 1:97], big_W[1:18, 1:97], big_a[1:41], candidates=C, required=R, **kw), full)


def test_resamples_chunks_and_selection_frequency():
    X, W, alpha, C, R, kw, full = independence_inputs()
    X, alpha, C, R = X[:17], alpha[:17], C[:17], R[:17]
    call = lambda Rn, **extra: sal.nb_assign_signatures(X, W, alpha, candidates=C, required=R, n_resamples=Rn, resample_seed=5,  # noqa: E731
                                                        keep_resamples=True, **kw, **extra)
    four, eight = call(4), call(8)
    same(four, full, rows_b=slice(0, 17))
    assert np.array_equal(four.exposures_resampled, eight.exposures_resampled[:4])
    small = call(8, chunk_bytes=17 * 96 * 8 * 3)
    assert small.timings["n_chunks"] == 3 and eight.timings["n_chunks"] == 1
    for name in ("exposures_resampled", "selection_frequency", "exposures_mean", "exposures_quantiles"):
        assert np.array_equal(getattr(small, name), getattr(eight, name)), name
    assert np.array_equal(eight.selection_frequency, (eight.exposures_resampled > 0).mean(axis=0))
    assert (eight.exposures_resampled[:, ~C] == 0.0).all()
    draws = sal.resample_counts(X, 8, 5)
    for r in (0, 7):
        member = sal.nb_assign_signatures(draws[r], W, alpha, candidates=C, required=R, **kw)
        assert np.array_equal(member.exposures, eight.exposures_resampled[r])


def test_converged_is_false_exactly_where_a_solve_hit_the_cap():
    X, W = nref.catalogue(16, 4, 96, seed=21)
    alpha = np.where(np.arange(16) % 2 == 0, 0.5, 1e4)
    solve = dict(min_iterations=10, max_iterations=60, conv_test_freq=10, tol=1e-4)
    got = sal.nb_assign_signatures(X, W, alpha, **solve)
    want = nar.assign(X, W, alpha, **solve)
    capped = got.n_iterations == 60 * (got.n_trials.astype(np.int64) + 1)
    print(f"converged {got.converged.sum()} of 16; dense converged {got.dense_converged.sum()}; replica converged {want.converged.sum()}")
    assert (got.dense_converged | (got.dense_n_iterations == 60)).all()
    assert not got.converged[capped].any()
    assert np.array_equal(got.converged, want.converged) and np.array_equal(got.n_iterations, want.n_iterations)
    assert got.converged.any() and not got.converged.all()


def test_the_c_entry_point_refuses_what_python_refuses():
    lib = _lib.load_with_device()
    N, K, V = 4, 3, 10
    X, W = nref.catalogue(N, K, V, seed=0)
    W = np.ascontiguousarray(W / W.sum(axis=1, keepdims=True))
    p = _lib.pointer

    def status(X=X, W=W, alpha=np.full(N, 20.0), max_it=20, cand=None, req=None, N=N, K=K, V=V):
        f64 = lambda *s: np.full(s, -7.0)  # noqa: E731
        i32 = lambda *s: np.full(s, -7, dtype=np.int32)  # noqa: E731
        out = [f64(N, K), i32(N, K), f64(N), i32(N, K), f64(N, K), i32(N), np.full(N, -7, dtype=np.int64), i32(N), f64(N, K), f64(N), i32(N), i32(N)]
        alpha = np.ascontiguousarray(alpha, dtype=np.float64)
        q = np.empty(0)
        rc = lib.salnmf_nb_assign_signatures(0, p(np.ascontiguousarray(X)), N, V, p(np.ascontiguousarray(W)), K, p(alpha), 0, 0, 0, p(q), 20, max_it, 5,
                                             1e-7, 1.92, 0, p(cand), p(req), 0, *(p(o) for o in out), None, None, None, None, None, None, None)
        assert all((o == -7).all() for o in out) or rc == 0
        return rc

    assert status() == 0
    for bad in (0.0, -1.0, np.inf, np.nan, 1e6 + 1):
        a = np.full(N, 20.0)
        a[2] = bad
        assert status(alpha=a) == 1
    assert status(max_it=22) == 1
    one = np.zeros((N, K), dtype=np.uint8)
    one[:, 0] = 1
    assert status(cand=one, req=np.ones((N, K), dtype=np.uint8)) == 1
    empty = np.ones((N, K), dtype=np.uint8)
    empty[1] = 0
    assert status(cand=empty) == 1
    assert status(X=np.ones((N, 97)), W=np.ones((K, 97)) / 97, V=97) == 1
    assert status(W=np.ones((97, V)) / V, K=97) == 1
    assert status(cand=one, req=one) == 0


def test_estimate_dispersion_on_candidate_sets():
    X, W = nref.recovery_data()
    X = X[:16]
    K = W.shape[0]
    grid = np.geomspace(2, 2e3, 5)
    solve = dict(min_iterations=50, max_iterations=200, conv_test_freq=10, tol=1e-6)
    plain = sal.estimate_dispersion(X, W, grid, **solve)
    every = sal.estimate_dispersion(X, W, grid, candidates=np.ones(K, dtype=bool), **solve)
    scale = np.stack([nar.row_scale(X, W, grid[a], plain.exposures[a]) for a in range(grid.size)])
    dP = float((np.abs(every.profile - plain.profile) / scale).max())
    dH = float((np.abs(every.exposures - plain.exposures) / np.maximum(plain.exposures, nar.EPSILON)).max())
    print(f"all candidates against none: profile {dP:.3g} tol {F_TOL:.3g}; exposures {dH:.3g} tol {H_TOL:.3g}")
    assert dP <= F_TOL and dH <= H_TOL
    assert every.dispersion == plain.dispersion and abs(every.lr_statistic - plain.lr_statistic) <= 2 * F_TOL * scale.sum()
    mask = np.array([True, True, False, True])
    shared = sal.estimate_dispersion(X, W, grid, candidates=mask, **solve)
    cut = sal.estimate_dispersion(X, W[mask], grid, **solve)
    scale = np.stack([nar.row_scale(X, W[mask], grid[a], cut.exposures[a]) for a in range(grid.size)])
    dP = float((np.abs(shared.profile - cut.profile) / scale).max())
    print(f"shared mask against the cut catalogue: profile {dP:.3g} tol {F_TOL:.3g}; dispersion {shared.dispersion} {cut.dispersion}")
    assert shared.dispersion == cut.dispersion and shared.at_upper_edge == cut.at_upper_edge and dP <= F_TOL
    assert (shared.exposures[:, :, ~mask] == 0.0).all() and (shared.exposures[:, :, mask] > 0.0).all()
    per, _ = amr.case_sets(16, K, 4, "random")
    own = sal.estimate_dispersion(X, W, grid, candidates=per, per_sample=True, **solve)
    assert np.array_equal(own.exposures == 0.0, np.broadcast_to(~per, (grid.size, 16, K)))
    assert own.dispersion.shape == (16,)
