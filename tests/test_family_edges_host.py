"""The CPU side of tests/test_gpu_family_edges.py: every yardstick that file holds the device to is measured here on the case's
own inputs, float64 replicas in two summation orders against longdouble, and every condition on the inputs is asserted -- the
decisions are isolated, the pivots are far from the threshold or exactly 0, and no case is vacuous (it has tested and untested
pairs, problems that stop at different tests, entries clipped at EPSILON)."""

import numpy as np
import pytest

import _assign_masks_ref as mref
import _assign_ref as aref
import _change_ref as change_ref
import _cov_ref as cov_ref
import _presence_ref as presence_ref
import _refit_ref as ref
import _sigchange_ref as sigchange_ref
import test_gpu_assign as tga
import test_gpu_covariance as tgc
import test_gpu_family_edges as edges
import test_gpu_refit as tgr

pytestmark = []  # (the imported modules' ``gpu`` marks are theirs: nothing here needs a device)
EPS = ref.EPSILON


def test_the_shapes_cover_every_instantiation_and_edge():
    kt = lambda K: (K + 15) // 16  # noqa: E731
    for k in range(1, 7):
        mine = sorted(K for K, _ in edges.SHAPES if kt(K) == k)
        assert mine and mine[-1] in (16 * k, 16 * k - 1) and (k < 3 or mine[0] == 16 * k - 15), k
        assert any(kt(K) == k for K, _ in edges.ONE_PER_KT)
    for group in ((1,), (15, 16, 17), (33,), (83,), (95,), (96,)):
        assert sum(V in group for _, V in edges.SHAPES) >= (2 if group not in ((1,), (33,)) else 1), group
    assert [K % 32 for K, _ in edges.WORD_EDGES] == [31, 0, 31, 0]
    assert {kt(K) for _, K in edges.CONVERGENCE} == {3, 5}


@pytest.mark.parametrize("K,V", edges.SHAPES)
def test_refit_spread_holds(K, V):
    X, W = edges.refit_case(K, V)
    ld, spread = tgr.host_spread(X, W, min_iterations=tgr.T, max_iterations=tgr.T)
    print(f"refit K={K} V={V}: host spread {spread:.3g} (recorded {tgr.H_SPREAD:.3g}), {int((ld.exposures == EPS).sum())} entries at the floor")
    assert spread <= tgr.H_SPREAD
    assert (ld.exposures == EPS).any() and (ld.exposures > EPS).any() and (X == 0.0).any() and not X[2].any() and X[1].sum() == 1.0


@pytest.mark.parametrize("P,K", edges.CONVERGENCE)
def test_refit_convergence_yardstick_holds(P, K):
    """The g of ``test_gpu_refit.test_convergence_of_every_problem`` on the case's inputs, over every eligible test up to
    max_iterations: the device test's window ends at the device's last stop, which cannot be later."""
    X, W = tgr.catalogue(P, K, seed=100 + K)
    kw = dict(min_iterations=500, max_iterations=4000, conv_test_freq=10, tol=1e-7)
    own = ref.refit(X, W, **kw)
    assert 1 < np.unique(own.n_iterations).size and own.converged.any()  # problems stop at different tests
    last = kw["max_iterations"]
    free = [ref.refit(X, W, free_run=True, **{**kw, "max_iterations": last}, **extra)
            for extra in (dict(dtype=np.longdouble), {}, dict(perm=np.random.default_rng(7).permutation(96)))]
    ld, tests = free[0], free[0].tests
    eligible = tests >= kw["min_iterations"]
    g_raw = 0.0
    for p in range(P):
        stop = next((t for t, c in zip(tests[eligible], ld.changes[eligible, p]) if c < kw["tol"]), last)
        m = eligible & (tests <= stop)
        for run in free[1:]:
            g_raw = max(g_raw, float((np.abs(run.changes[m, p] - ld.changes[m, p]) / np.maximum(ld.changes[m, p], kw["tol"])).max(initial=0.0)))
    print(f"convergence N={P} K={K}: g_raw {g_raw:.3g} (recorded {tgr.G_RAW:.3g})")
    assert g_raw <= tgr.G_RAW


def f_bound(K, V, kind):
    return max(mref.F_SPREAD, edges.F_SPREAD_OF.get((K, V, kind), 0.0))


@pytest.mark.parametrize("K,V", edges.ASSIGN_SHAPES)
def test_plain_assignment_cases_are_isolated(K, V):
    X, W, runs = tga.replicas(*edges.plain_case(K, V))
    ok, margin = aref.isolation(runs, edges.THR)
    _, h_spread, f_spread = tga.host_spread(X, W, runs)
    print(f"assign K={K} V={V}: isolated {ok.sum()} of {ok.size}, threshold margin {margin:.3g}, host spread H {h_spread:.3g} f {f_spread:.3g}")
    assert ok.all()
    assert h_spread <= mref.H_SPREAD and f_spread <= f_bound(K, V, "plain")
    assert runs[0].n_trials.min() >= 1 and not runs[0].active.all()


@pytest.mark.parametrize("K,V", edges.ASSIGN_SHAPES + edges.WORD_EDGES)
def test_masked_assignment_cases_are_isolated(K, V):
    X, W, kw, runs, (ok, margin, umargin) = mref.case_replicas(*edges.masked_case(K, V))
    rows = np.flatnonzero(ok)
    _, h_spread, f_spread = mref.host_spread(X, W, runs, rows)
    print(f"masks K={K} V={V}: isolated {ok.sum()} of {ok.size}, threshold margin {margin:.3g}, u margin {umargin:.3g}, host spread H {h_spread:.3g} "
          f"f {f_spread:.3g}")
    assert ok.sum() >= 0.9 * ok.size
    assert h_spread <= mref.H_SPREAD and f_spread <= f_bound(K, V, "masked")
    C = kw["candidates"]
    assert C[:, K - 1].all() and C[:, 32 * ((K - 1) // 32)].all() and not C.all(axis=1).any()
    assert 1 < np.unique(runs[0].n_trials).size and any(t["kind"] == "add" for ts in runs[0].trials for t in ts)


def test_phase_zero_spread_at_a_single_feature():
    K, V = edges.SHAPES[0]
    X, W, ld, _, h_spread, f_spread = edges.phase_zero_reference(K, V)
    print(f"assign phase 0 K={K} V={V}: host spread H {h_spread:.3g} f {f_spread:.3g}")
    assert V == 1 and h_spread <= mref.H_SPREAD and f_spread <= mref.F_SPREAD
    assert (X > 0.0).any() and (ld.exposures > EPS).any()
    C, _ = mref.case_sets(edges.N, K, 0, "edge")
    assert C[:, [0, K - 1]].all() and not C.all(axis=1).any()


@pytest.mark.parametrize("K,V", edges.SHAPES + edges.WORD_EDGES)
def test_exposure_change_cases(K, V):
    """The inputs of ``test_exposure_change_against_the_replica``: tested and untested pairs, the candidate-word edge in every
    set, fits that stop at different tests, and the float64 spread of the null divergences within its record."""
    Xa, Xb, W, C = change_ref.gpu_case(K, V)
    t = change_ref.tested_pairs(Xa, Xb, C)
    assert not t[[0, 5, 9]].any() and t[1:5].all() and t[10:].all()
    assert C[t][:, [1, K - 1, 32 * ((K - 1) // 32)]].all() and not C[10:].all() and (W[K - 1] == 0.0).any() == (V > 1)
    assert [Xa[r].sum() for r in range(5)] == [0.0, 1.0, 2.0, 257.0, 100000.0] and [Xb[r].sum() for r in range(1, 6)] == [257.0, 1.0, 100000.0, 2.0, 0.0]
    rows = np.flatnonzero(t)
    pooled = np.maximum(Xa[rows], EPS) + np.maximum(Xb[rows], EPS)
    fits = [presence_ref.solve(X, W, C[rows], **change_ref.GPU_FIT) for X in (Xa[rows], Xb[rows], pooled)]
    nit, conv = np.stack([f.n_iterations for f in fits]), np.stack([f.converged for f in fits])
    assert 1 < np.unique(nit).size and conv.any() and not conv.all()  # problems stop at different tests
    assert (fits[2].exposures[C[rows]] == EPS).any() or V == 1  # entries clipped at the floor
    g = change_ref.g_spread(K, V)
    print(f"change K={K} V={V}: {rows.size} tested pairs, iterations {np.unique(nit)}, host spread g {g:.3g} (recorded {change_ref.G_SPREAD:.3g})")
    assert g <= max(change_ref.G_SPREAD, edges.CHANGE_G_SPREAD_OF.get((K, V), 0.0))


@pytest.mark.parametrize("K,V", edges.SHAPES + edges.WORD_EDGES)
def test_signature_change_cases(K, V):
    """The inputs of ``test_signature_change_against_the_replica``: the tested signatures, tested and untested problems in several
    tiles of 8, most tied entries off the floor and some on it, and the tied solve's float64 spread
    within its record."""
    Xa, Xb, W, C, test = sigchange_ref.gpu_case(K, V)
    assert test == tuple(sorted({0, 32 * ((K - 1) // 32), K - 1})) and len(test) >= 2
    t = sigchange_ref.tested_problems(Xa, Xb, C, test)
    ns, js, sig = sigchange_ref.gpu_problems(K, V)
    assert not t[[0, 5, 9]].any() and t[1:5].all() and t[10:, -1].all()
    assert (~t[10:]).any() == (K > 32)  # (up to K = 32 signature 0 is bit 0 of the last word, and in every set)
    assert ns.size > 16  # (the last tile is partly filled at all shapes but (40, 96), (70, 96) and (63, 96): 104 problems)
    dh, df, ld, _ = sigchange_ref.fixed_spread(K, V)
    at = np.arange(ns.size)
    off = (ld.exposures_a[at, sig] > EPS) & (ld.exposures_b[at, sig] > EPS)
    assert off.sum() >= ns.size // 2
    assert (ld.exposures_a[C[ns]] == EPS).any() or V == 1  # entries clipped at the floor
    print(f"sigchange K={K} V={V}: test {test}, {ns.size} problems, {int(off.sum())} off the floor, host spread H {dh:.3g} f {df:.3g} "
          f"(recorded {sigchange_ref.H_SPREAD:.3g} {sigchange_ref.F_SPREAD:.3g})")
    assert dh <= max(sigchange_ref.H_SPREAD, edges.SIGCHANGE_SPREAD_OF.get((K, V, "h"), 0.0))
    assert df <= max(sigchange_ref.F_SPREAD, edges.SIGCHANGE_SPREAD_OF.get((K, V, "f"), 0.0))


@pytest.mark.parametrize("K,V", edges.SHAPES + edges.WORD_EDGES)
def test_pair_cases(K, V):
    X, W, test, C = edges.pair_case(K, V)
    assert test == [0, K - 1] and np.allclose(W.sum(axis=1), 1.0) and (W[K - 1] == 0.0).any() == (V > 1)
    t = presence_ref.tested_pairs(C, test)
    assert t[:5].all() and not t[5:9, 0].any() and t[5:9, 1].all() and not t[9].any() and not t[10].any() and t[11:].all()
    assert C[11:, [K - 1, 32 * ((K - 1) // 32)]].all() and not C[11:].all()
    assert X[:5].sum(axis=1).tolist() == [0.0, 1.0, 2.0, 257.0, 100000.0]
    # the fixed solves' float64 spread about longdouble, on the alternative fits and on the null fits of both tested signatures
    worst_h = worst_f = 0.0
    for s in (None, *test):
        rows = np.flatnonzero(t.any(axis=1) if s is None else t[:, test.index(s)])
        sets = C[rows].copy()
        if s is not None:
            sets[:, s] = False
        runs = mref.three_runs(X[rows], W, solve=edges.STEPS, candidates=sets, required=sets)
        _, h, f = mref.host_spread(X[rows], W, runs)
        worst_h, worst_f = max(worst_h, h), max(worst_f, f)
        if s is None:
            assert (runs[2].exposures[sets] == EPS).any()  # entries clipped at the floor
    print(f"pairs K={K} V={V}: host spread H {worst_h:.3g} f {worst_f:.3g}")
    assert worst_h <= mref.H_SPREAD and worst_f <= f_bound(K, V, "pair")
    if V > 1:  # (with one feature every solve sits at its fixed point after one step)
        rows = np.flatnonzero(t.any(axis=1))
        assert 1 < np.unique(presence_ref.solve(X[rows], W, C[rows], **edges.FIT).n_iterations).size


@pytest.mark.parametrize("information", tgc.INFORMATION)
@pytest.mark.parametrize("K,V", edges.SHAPES)
def test_covariance_records_hold(K, V, information):
    X, W, H, active = edges.cov_case(K, V)
    r = edges.cov_reference(K, V, information)  # (asserts the pivot conditions)
    rel, absolute = cov_ref.measure(X, W, H, active, information, ref=r)
    record = edges.COV_MEASURED[K, V, information]
    print(f"    ({K}, {V}, \"{information}\"): ({rel:.2g}, {absolute:.2g}),  # recorded {record}, {int(r.singular.sum())} singular")
    assert rel <= record[0] and absolute <= record[1]
    if K > V:
        assert (active[2:].sum(axis=1) <= min(V, 5)).all() and r.singular[:2].all() and not r.singular[2:].any()
    else:
        assert not r.singular.any() and (r.n_active == 0).any() and (r.n_active == K).any()


@pytest.mark.parametrize("K,V", edges.PAD_SHAPES)
def test_appended_zero_features_are_no_no_op_of_the_contract(K, V):
    """All-zero features appended to the counts and to the signatures: the contract clips the zero count to EPSILON, the zero
    signature column gives (h W)_v = 0, and the step's EPSILON / 0 times the zero entry is NaN -- in every replica, so the
    device test compares nothing of such a call."""
    X, W = edges.refit_case(K, V)
    Xz, Wz = np.hstack([X, np.zeros((X.shape[0], 3))]), np.hstack([W, np.zeros((K, 3))])
    with np.errstate(all="ignore"):
        wide = ref.refit(Xz, Wz, min_iterations=20, max_iterations=20)
    assert np.isnan(wide.exposures).all() and not np.isfinite(wide.reconstruction_errors).any()
