"""Candidate sets, required signatures and the re-addition pass of ``sal.assign_signatures`` without a device (DESIGN.md
section 14.1): what is refused before a device is touched, on either side of the C ABI; the replica
(tests/_assign_masks_ref.py) against the replica of section 14 (tests/_assign_ref.py); and the isolation of every decision of
the cases tests/test_gpu_assign_masks.py compares exactly."""

import numpy as np
import pytest

import _assign_masks_ref as mref
import _assign_ref as aref
import _refit_ref as ref
import salamander_amd as sal
from salamander_amd import _lib
from salamander_amd import assign as assign_mod

NAMES = ("exposures", "active", "reconstruction_errors", "removal_round", "kl_increase", "n_trials", "n_iterations", "converged")
DENSE = ("exposures", "reconstruction_errors", "n_iterations", "converged")


def same(a, b):
    for name in NAMES:
        assert np.array_equal(getattr(a, name), getattr(b, name), equal_nan=True), name
    for name in DENSE:
        assert np.array_equal(getattr(a.dense, name), getattr(b.dense, name)), "dense " + name


def test_python_refuses_bad_sets_before_the_device(monkeypatch):
    def no_device(*a, **k):
        raise AssertionError("the library was loaded")

    monkeypatch.setattr(assign_mod._lib, "load", no_device)
    X, W = ref.poisson_catalogue(4, 3, V=10, seed=0)
    yes, no = np.ones(3, dtype=bool), np.zeros(3, dtype=bool)
    one = np.array([True, False, False])
    empty_row = np.ones((4, 3), dtype=bool)
    empty_row[2] = False
    bad = [dict(candidates=np.ones(4, dtype=bool)), dict(candidates=np.ones((3, 4), dtype=bool)), dict(candidates=np.ones((4, 3, 1), dtype=bool)),
           dict(candidates=np.ones(3)), dict(candidates=np.ones(3, dtype=np.uint8)), dict(candidates=[1, 1, 1]), dict(candidates=no),
           dict(candidates=empty_row), dict(required=np.ones(2, dtype=bool)), dict(required=np.ones((4, 3))), dict(candidates=one, required=yes),
           dict(candidates=one, required=np.array([False, True, False])), dict(readd=1), dict(readd=None), dict(readd="yes")]
    for kw in bad:
        with pytest.raises(ValueError):
            sal.assign_signatures(X, W, max_iterations=1000, **kw)
    good = [dict(candidates=yes, required=no, readd=False), dict(candidates=one, required=one, readd=True), dict(candidates=[True, False, True]),
            dict(candidates=np.ones((4, 3), dtype=bool), required=np.zeros((4, 3), dtype=bool)), dict(required=yes), dict(readd=np.True_)]
    for kw in good:  # a valid call gets as far as the library
        with pytest.raises(AssertionError, match="library was loaded"):
            sal.assign_signatures(X, W, max_iterations=1000, **kw)
    C, R, readd = assign_mod.check_sets(one, None, True, 4, 3)
    assert C.shape == (4, 3) and C.dtype == np.bool_ and R is None and readd is True and np.array_equal(C, np.tile(one, (4, 1)))
    for kw in (dict(candidates=no), dict(candidates=one, required=yes)):
        with pytest.raises(ValueError):
            mref.assign(X, W, max_iterations=10, **kw)


def test_c_abi_refuses_bad_sets_on_the_host():
    """The library loads without a device, and the shared routine refuses the sets before it opens one: status 1 and a message
    that names the sample."""
    lib = _lib.load()
    N, V, K = 4, 10, 3
    X, W = ref.poisson_catalogue(N, K, V=V, seed=0)
    X, W = np.ascontiguousarray(X), np.ascontiguousarray(W)
    f64 = lambda *shape: np.zeros(shape, dtype=np.float64)  # noqa: E731
    i32 = lambda *shape: np.zeros(shape, dtype=np.int32)  # noqa: E731
    out = dict(H=f64(N, K), act=i32(N, K), err=f64(N), rnd=i32(N, K), kl=f64(N, K), ntr=i32(N), nit=np.zeros(N, dtype=np.int64), conv=i32(N),
               Hd=f64(N, K), err_d=f64(N), nit_d=i32(N), conv_d=i32(N), rrnd=i32(N, K), kld=f64(N, K))
    p = _lib.pointer

    def call(candidates, required, readd, outputs=True):
        u8 = lambda m: None if m is None else np.ascontiguousarray(m, dtype=np.uint8)  # noqa: E731
        C, R = u8(candidates), u8(required)
        rc = lib.salnmf_assign_signatures_ex(0, p(X), N, V, p(W), K, 0, 0, 0, None, 20, 20, 5, 1e-7, 1.92, 0, p(C), p(R), readd,
                                             p(out["H"]), p(out["act"]), p(out["err"]), p(out["rnd"]), p(out["kl"]), p(out["ntr"]), p(out["nit"]),
                                             p(out["conv"]), p(out["Hd"]), p(out["err_d"]), p(out["nit_d"]), p(out["conv_d"]), None, None, None, None,
                                             p(out["rrnd"]) if outputs else None, p(out["kld"]) if outputs else None, None)
        return rc, _lib.last_error()

    empty_row = np.ones((N, K), dtype=bool)
    empty_row[2] = False
    rc, msg = call(empty_row, None, 0)
    assert rc == 1 and "sample 2 has no candidate" in msg
    C = np.ones((N, K), dtype=bool)
    C[3, 1] = False
    R = np.zeros((N, K), dtype=bool)
    R[3, 1] = True
    rc, msg = call(C, R, 0)
    assert rc == 1 and "sample 3" in msg and "required signature 1 is not a candidate" in msg
    for readd in (2, -1):
        rc, msg = call(None, None, readd)
        assert rc == 1 and "readd must be 0 or 1" in msg
    rc, msg = call(None, None, 1, outputs=False)
    assert rc == 1 and "null output for the re-addition pass" in msg


def test_without_sets_the_replica_is_the_replica_of_section_14():
    X, W = ref.poisson_catalogue(20, 6, seed=2, zero_heavy=2)
    for kw in (dict(min_iterations=20, max_iterations=200, conv_test_freq=10, tol=1e-5), mref.FIXED):
        want = aref.assign(X, W, **kw)
        for sets in (dict(), dict(candidates=np.ones(6, dtype=bool), required=np.zeros((20, 6), dtype=bool), readd=False)):
            got = mref.assign(X, W, **kw, **sets)
            same(got, want)
            assert (got.readd_round == -1).all() and np.isnan(got.kl_decrease).all()


@pytest.mark.parametrize("case", [c for c in mref.CASES if c[4] != "required"], ids=str)
def test_restriction_to_candidates_is_the_sub_catalogue_exactly(case):
    """The independent check of the mask semantics: the old replica on ``signatures[C_n]``, row by row, scattered back."""
    X, W, kw = mref.case_inputs(*case)
    got = mref.assign(X, W, kw["max_kl_increase"], candidates=kw["candidates"], **mref.FIXED)
    want = mref.on_subcatalogue(X, W, kw["candidates"], max_kl_increase=kw["max_kl_increase"], **mref.FIXED)
    same(got, want)
    assert (got.exposures[~got.candidates] == 0.0).all() and not got.active[~got.candidates].any()
    assert np.isnan(got.kl_increase[~got.candidates]).all() and (got.dense.exposures[~got.candidates] == 0.0).all()


def test_a_required_signature_is_never_tried():
    for case in (c for c in mref.CASES if c[4] == "required"):
        X, W, kw, runs, _ = mref.case_replicas(*case)
        got = runs[0]
        R = got.required
        assert R.any(axis=1).all() and not (R & ~got.candidates).any()
        assert got.active[R].all() and (got.removal_round[R] == -1).all() and np.isnan(got.kl_increase[R]).all() and (got.exposures[R] > 0).all()
        assert all(t["candidate"] >= 0 and not R[p, t["candidate"]] for p, ts in enumerate(got.trials) for t in ts if t["kind"] != "select" or t["go"])
        free = mref.assign(X, W, kw["max_kl_increase"], candidates=kw["candidates"], readd=kw["readd"], **mref.FIXED)
        assert (~free.active & R).any()  # without the requirement some of them are removed: the requirement does something


def readd_properties(X, W, got, thr):
    """What the contract promises of a finished re-addition pass, read off a replica run."""
    x = np.maximum(X, mref.EPSILON)
    accepted = 0
    for p, ts in enumerate(got.trials):
        kinds = [t["kind"] for t in ts]
        first_select = kinds.index("select")
        assert "remove" not in kinds[first_select:]  # no second backward pass
        last = ts[-1]
        assert last["kind"] == "select" and not last["go"]  # the pass ends on a selection that does not go
        pool = got.candidates[p] & ~got.active[p]
        tried = np.zeros_like(pool)
        tried[[t["candidate"] for t in ts if t["kind"] == "add"]] = True
        assert not (tried & ~got.candidates[p]).any() and sum(k == "add" for k in kinds) == tried.sum()  # each at most once
        u = mref.update_factors(x[p:p + 1], W, got.exposures[p:p + 1])[0]
        assert (u[pool & ~tried] <= 1.0).all()  # KKT at every untried zero, or every pool member tried
        for t in ts:
            if t["kind"] == "add":
                assert t["accepted"] == bool(t["delta"] > thr)
                assert got.kl_decrease[p, t["candidate"]] == t["delta"]
                assert (got.readd_round[p, t["candidate"]] >= 0) == t["accepted"]
                accepted += t["accepted"]
        back = got.removal_round[p][got.readd_round[p] >= 0]
        assert (back >= 0).all()  # a re-added signature had been removed, and keeps that round
        assert got.active[p][got.readd_round[p] >= 0].all()
        assert got.n_trials[p] == sum(k in ("remove", "add") for k in kinds)
    return accepted


def test_the_re_addition_pass_on_the_replica():
    total = 0
    for case in (c for c in mref.CASES if c[5]):
        X, W, kw, runs, _ = mref.case_replicas(*case)
        total += readd_properties(X, W, runs[0], kw["max_kl_increase"])
        back = mref.assign(X, W, kw["max_kl_increase"], candidates=kw["candidates"], required=kw["required"], **mref.FIXED)
        # the backward rounds are the same with and without the pass
        assert np.array_equal(back.removal_round, runs[0].removal_round) and np.array_equal(back.kl_increase, runs[0].kl_increase, equal_nan=True)
    assert total >= 2  # the cases at the thresholds 0.1 and -0.01 accept one each


def test_planted_catalogue_with_the_re_addition_pass():
    """Section 14's planted-recovery generator (3 of 12 Dirichlet(0.15) signatures, 450 to 3 500 mutations, T = 200, threshold
    1.92).  Searched on the CPU over seeds 0..99 for a row where the backward rounds lose a planted signature and the
    re-addition pass restores it: there is none -- the backward rounds keep every planted signature in all 1 200 rows, so
    the pass has nothing planted to restore.  It tried 3 194 signatures and accepted 9, in the seeds 14, 21, 36, 49, 50, 74, 85
    (one each) and 94 (two); seed 94 is committed as the case in which the pass changes the answer."""
    X, W, planted = aref.planted_catalogue(seed=mref.PLANTED_SEED)
    kw = dict(min_iterations=200, max_iterations=200, conv_test_freq=10)
    back = mref.assign(X, W, 1.92, **kw)
    both = mref.assign(X, W, 1.92, readd=True, **kw)
    assert (back.active | ~planted).all() and (both.active | ~planted).all()
    assert readd_properties(X, W, both, 1.92) == 2 and (both.readd_round >= 0).sum() == 2
    rows = (both.readd_round >= 0).any(axis=1)
    assert (both.reconstruction_errors[rows] < back.reconstruction_errors[rows] - 1.92).all()
    assert np.array_equal(both.active[~rows], back.active[~rows]) and np.array_equal(both.exposures[~rows], back.exposures[~rows])


@pytest.mark.parametrize("case", mref.CASES, ids=str)
def test_every_decision_of_the_gpu_cases_is_isolated(case):
    """The float64 replica in two feature orders and the longdouble replica take the same decisions; every threshold
    comparison, in both directions, clears its threshold by 1e-6 max(1, |threshold|), every u_c clears 1 by 1e-6, every arg-min
    winner is bit-equal to EPSILON or a relative 1e-6 below the runner-up, every arg-max winner a relative 1e-6 above it.  The
    host spreads these cases give stay within the recorded constants the device's bounds are built on."""
    X, W, kw, runs, (ok, margin, umargin) = mref.case_replicas(*case)
    rows = np.flatnonzero(ok)
    _, h_spread, f_spread = mref.host_spread(X, W, runs, rows)
    print(f"{case}: isolated {ok.sum()} of {ok.size}, threshold margin {margin:.3g}, u margin {umargin:.3g}, host spread H {h_spread:.3g} f {f_spread:.3g}")
    assert ok.sum() >= 0.9 * ok.size
    assert h_spread <= mref.H_SPREAD and f_spread <= mref.F_SPREAD
