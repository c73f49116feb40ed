"""``sal.nb_assign_signatures`` without a device: the replica (tests/_nb_assign_ref.py) against the
replica of the dense refit (tests/_nb_ref.py), the isolation of every decision of the cases tests/test_gpu_nb_assign.py compares
exactly, the host spreads the device's tolerances are built from, what Python refuses before a device is touched, and one
statistical sanity check of the procedure on the replica."""

import numpy as np
import pytest

import _assign_masks_ref as amr
import _nb_assign_ref as nar
import _nb_ref as nref
import salamander_amd as sal
from salamander_amd import nb as nb_mod


@pytest.mark.parametrize("case", nar.CASES, ids=lambda c: f"P{c[0]}-K{c[1]}-V{c[2]}-{c[4]}")
def test_cases_are_isolated_and_within_the_recorded_spreads(case):
    X, W, alpha, kw, runs, (ok, margin, umargin) = nar.case_replicas(*case)
    rows = np.flatnonzero(ok)
    _, dH, dF = nar.host_spread(X, W, alpha, runs, rows)
    print(f"{case}: isolated {ok.sum()} of {ok.size}, threshold margin {margin:.3g}, u margin {umargin:.3g}, H spread {dH:.3g}, f spread {dF:.3g}")
    assert ok.mean() >= nar.MIN_ISOLATED
    assert dH <= nar.H_SPREAD and dF <= nar.F_SPREAD
    for run in runs:
        assert np.array_equal(run.exposures == 0.0, ~run.active)
        assert not run.active[~run.candidates].any() and run.active[run.required].all()
        assert np.isnan(run.kl_increase.astype(np.float64)[run.required]).all()


def test_two_cases_accept_a_re_addition():
    accepting = [i for i in nar.READD_CASES if (nar.case_replicas(*nar.CASES[i])[4][2].readd_round >= 0).any()]
    print("cases with an accepted re-addition:", [nar.CASES[i] for i in accepting])
    assert len(accepting) >= 2


@pytest.mark.parametrize("K,V", [(3, 7), (17, 96)])
def test_phase_0_is_the_dense_replica_bit_for_bit(K, V):
    X, W = nref.catalogue(17, K, V, seed=3)
    alpha = nref.mixed_alpha(17)
    for solve in (amr.FIXED, dict(min_iterations=30, max_iterations=200, conv_test_freq=10, tol=1e-5)):
        got = nar.assign(X, W, alpha, **solve)
        want = nref.nb_refit(X, W, alpha, **solve)
        assert np.array_equal(got.dense.exposures, want.exposures)
        assert np.array_equal(got.dense.reconstruction_errors, want.reconstruction_errors)
        assert np.array_equal(got.dense.n_iterations, want.n_iterations) and np.array_equal(got.dense.converged, want.converged)


def test_an_active_set_solve_takes_no_trial():
    X, W = nref.catalogue(17, 17, 96, seed=5)
    alpha = nref.mixed_alpha(17)
    A, _ = amr.case_sets(17, 17, 5, "random")
    for readd in (False, True):
        got = nar.assign(X, W, alpha, candidates=A, required=A, readd=readd, **amr.FIXED)
        assert not got.n_trials.any() and np.array_equal(got.active, A) and np.array_equal(got.exposures, got.dense.exposures)
        assert np.array_equal(got.exposures == 0.0, ~A) and np.array_equal(got.n_iterations, np.full(17, 20))
        assert all(t["kind"] == "select" and t["candidate"] == -1 for row in got.trials for t in row)


def test_python_refuses_before_the_device(monkeypatch):
    def no_device(*a, **k):
        raise AssertionError("the library was loaded")

    monkeypatch.setattr(nb_mod._lib, "load", no_device)
    X, W = nref.catalogue(4, 3, 10, seed=0)
    one = np.array([True, False, False])
    bad = [dict(dispersion=0.0), dict(dispersion=-1.0), dict(dispersion=np.inf), dict(dispersion=np.nan), dict(dispersion=1e6 + 1),
           dict(dispersion=[1.0, 2.0]), dict(max_iterations=1005), dict(max_kl_increase=np.nan), dict(max_kl_increase=True),
           dict(candidates=np.zeros(3, dtype=bool)), dict(candidates=np.ones(3)), dict(candidates=one, required=np.ones(3, dtype=bool)),
           dict(readd=1), dict(n_resamples=-1), dict(tol=-1.0)]
    for kw in bad:
        args = {"dispersion": 20.0, "max_iterations": 1000, **kw}
        with pytest.raises(ValueError):
            sal.nb_assign_signatures(X, W, **args)
    with pytest.raises(ValueError):
        sal.nb_assign_signatures(np.ones((2, 97)), np.ones((3, 97)), 20.0)
    with pytest.raises(ValueError):
        sal.nb_assign_signatures(np.ones((2, 9)), np.ones((97, 9)), 20.0)
    for kw in (dict(), dict(candidates=one, required=one, readd=True), dict(dispersion=[0.5, 20.0, 1e4, 1e6])):
        args = {"dispersion": 20.0, "max_iterations": 1000, **kw}
        with pytest.raises(AssertionError, match="library was loaded"):  # a valid call gets as far as the library
            sal.nb_assign_signatures(X, W, **args)
    for kw in (dict(candidates=np.zeros(3, dtype=bool)), dict(candidates=np.ones((2, 3), dtype=bool)), dict(candidates=np.ones(3)),
               dict(candidates=one, max_iterations=1005)):
        with pytest.raises(ValueError):
            sal.estimate_dispersion(X, W, **kw)
    with pytest.raises(AssertionError, match="library was loaded"):
        sal.estimate_dispersion(X, W, candidates=one)


def test_the_c_entry_point_is_exported_and_bound():
    from salamander_amd import _lib

    lib = _lib.load()  # loads without a device
    ex, nb = _lib.SIGNATURES["salnmf_assign_signatures_ex"][1], _lib.SIGNATURES["salnmf_nb_assign_signatures"][1]
    assert nb[:6] == ex[:6] and nb[6] is _lib._D and nb[7:] == ex[6:]
    assert lib.salnmf_nb_assign_signatures.argtypes == nb


def test_planted_signatures_stay_under_the_true_dispersion():
    """Sanity of the procedure on the replica, not a gate on the device: gamma-Poisson counts (alpha = 20) of 3 planted signatures,
    12 offered.  Every planted signature with at least a tenth of its sample's mutations stays; the numbers of unplanted
    signatures kept are printed (DESIGN.md section 25 quotes them)."""
    X, W, E = nar.planted_catalogue()
    solve = dict(min_iterations=50, max_iterations=1000, conv_test_freq=10, tol=1e-6)
    nb = nar.assign(X, W, 20.0, **solve)
    poisson = amr.assign(X, W, **solve)
    big = E / E.sum(axis=1, keepdims=True) >= 0.1
    print(f"unplanted signatures kept in {X.shape[0]} samples x 9: negative binomial {int(nb.active[:, 3:].sum())}, Poisson {int(poisson.active[:, 3:].sum())}")
    assert nb.active[:, :3][big].all()
