"""``sal.assign_signatures`` with candidate sets, required signatures and the re-addition pass on the device (DESIGN.md section
14.1) against the host replica (tests/_assign_masks_ref.py) and against itself.

Decisions are compared exactly on the rows whose decisions tests/test_assign_masks_host.py shows isolated on the CPU (at
least 90 % of every case; all of them at the committed seeds).  Values are held to 16 x the spread of the two float64 feature
orders about the longdouble replica, measured on the CPU on these cases (``_assign_masks_ref.H_SPREAD`` / ``F_SPREAD``), never
to anything read off the device.
"""

import numpy as np
import pytest

import _assign_masks_ref as mref
import _assign_ref as aref
import _refit_ref as ref
import salamander_amd as sal
from salamander_amd import _lib

pytestmark = pytest.mark.gpu

EPS = ref.EPSILON
FIXED = mref.FIXED
NAMES = ("exposures", "active", "reconstruction_errors", "removal_round", "kl_increase", "n_trials", "n_iterations", "converged", "dense_exposures",
         "dense_errors", "dense_n_iterations", "dense_converged")
READD = ("readd_round", "kl_decrease")
RESAMPLED = ("selection_frequency", "exposures_mean", "exposures_quantiles", "exposures_resampled")
CONVERGING = dict(min_iterations=30, max_iterations=200, conv_test_freq=10, tol=1e-5)


def same(a, b, names=NAMES, rows=None):
    for name in names:
        x, y = getattr(a, name), getattr(b, name)
        if rows is not None:
            y = y[rows]
        assert np.array_equal(x, y, equal_nan=True), name


# ---- no change of existing behaviour

@pytest.mark.parametrize("P,K,kw", [(40, 5, CONVERGING), (17, 33, FIXED), (16, 96, FIXED)])
def test_default_sets_change_nothing(P, K, kw):
    X, W = ref.poisson_catalogue(P, K, seed=30 + K, zero_heavy=2)
    more = dict(n_resamples=4, resample_seed=3, keep_resamples=True, **kw)
    base = sal.assign_signatures(X, W, **more)
    assert base.readd_round is None and base.kl_decrease is None and base.candidates is None and base.required is None
    for sets in (dict(candidates=None, required=None, readd=False), dict(candidates=np.ones(K, dtype=bool)), dict(required=np.zeros(K, dtype=bool)),
                 dict(candidates=np.ones((P, K), dtype=bool), required=np.zeros((P, K), dtype=bool))):
        got = sal.assign_signatures(X, W, **more, **sets)
        same(got, base, NAMES + RESAMPLED)


def c_call(lib, ex, X, W, R, kw):
    N, V = X.shape
    K = W.shape[0]
    f64 = lambda *shape: np.full(shape, -7.0, dtype=np.float64)  # noqa: E731
    i32 = lambda *shape: np.full(shape, -7, dtype=np.int32)  # noqa: E731
    o = dict(exposures=f64(N, K), active=i32(N, K), errors=f64(N), removal_round=i32(N, K), kl_increase=f64(N, K), n_trials=i32(N),
             n_iterations=np.full(N, -7, dtype=np.int64), converged=i32(N), dense_exposures=f64(N, K), dense_errors=f64(N), dense_n_iterations=i32(N),
             dense_converged=i32(N), selection_frequency=f64(N, K), exposures_quantiles=f64(2, N, K), exposures_mean=f64(N, K),
             exposures_resampled=f64(max(R, 1), N, K))
    q = np.array([0.25, 0.75])
    p = _lib.pointer
    head = (0, p(X), N, V, p(W), K, R, 5, 2 if R else 0, p(q), kw["min_iterations"], kw["max_iterations"], kw["conv_test_freq"], 1e-7, 1.92, 0)
    outs = tuple(p(v) for v in o.values())
    if ex:
        _lib.check(lib.salnmf_assign_signatures_ex(*head, None, None, 0, *outs, None, None, None))
    else:
        _lib.check(lib.salnmf_assign_signatures(*head, *outs, None))
    return o


@pytest.mark.parametrize("R", [0, 4])
def test_the_old_entry_point_is_the_new_one_without_sets(R):
    lib = _lib.load_with_device()
    X, W = ref.poisson_catalogue(37, 17, seed=8, zero_heavy=2)
    X, W = np.ascontiguousarray(X), np.ascontiguousarray(W)
    old, new = c_call(lib, False, X, W, R, FIXED), c_call(lib, True, X, W, R, FIXED)
    for name in old:
        if R == 0 and name in ("selection_frequency", "exposures_quantiles", "exposures_mean", "exposures_resampled"):
            assert (old[name] == -7.0).all() and (new[name] == -7.0).all()  # not written without resamples
        else:
            assert np.array_equal(old[name], new[name], equal_nan=True) and not (old[name] == -7).all(), name


# ---- masks and re-addition against the replica

def sub_refit(X, W, C, kw):
    """``refit_exposures`` on the sub-catalogue of every distinct candidate set, scattered back."""
    P, K = X.shape[0], W.shape[0]
    H, err, nit, conv = np.zeros((P, K)), np.zeros(P), np.zeros(P, dtype=np.int32), np.zeros(P, dtype=bool)
    sets, which = np.unique(C, axis=0, return_inverse=True)
    which = np.asarray(which).reshape(-1)
    for i, c in enumerate(sets):
        rows, idx = np.flatnonzero(which == i), np.flatnonzero(c)
        r = sal.refit_exposures(X[rows], W[idx], **kw)
        H[np.ix_(rows, idx)] = r.exposures
        err[rows], nit[rows], conv[rows] = r.reconstruction_errors, r.n_iterations, r.converged
    return H, err, nit, conv


@pytest.mark.parametrize("case", mref.CASES, ids=str)
def test_decisions_and_values_against_the_replica(case):
    P, K = case[0], case[1]
    X, W, kw, runs, (ok, margin, umargin) = mref.case_replicas(*case)
    a, _, ld = runs
    assert ok.sum() >= 0.9 * ok.size
    rows = np.flatnonzero(ok)
    scale, h_spread, f_spread = mref.host_spread(X, W, runs, rows)
    got = sal.assign_signatures(X, W, **kw, **FIXED)
    C = np.broadcast_to(kw["candidates"], (P, K))
    assert np.array_equal(got.candidates, C)
    # 1. decisions, exactly
    for name in ("active", "removal_round", "n_trials", "n_iterations"):
        assert np.array_equal(getattr(got, name)[rows], getattr(a, name)[rows]), name
    assert np.array_equal(got.n_iterations, 20 * (got.n_trials.astype(np.int64) + 1))
    # (`converged` is every solve's last tolerance test: compared where the three replicas agree on it, which is every row here)
    agree = ok & (runs[0].converged == runs[1].converged) & (runs[0].converged == runs[2].converged)
    assert agree.sum() >= 0.9 * agree.size and np.array_equal(got.converged[agree], a.converged[agree])
    none = got.n_trials == 0
    assert np.array_equal(got.converged[none], got.dense_converged[none])
    if kw["readd"]:
        assert np.array_equal(got.readd_round[rows], a.readd_round[rows])
        assert np.array_equal(np.isnan(got.kl_decrease[rows]), np.isnan(a.kl_decrease[rows]))
    else:
        assert got.readd_round is None and got.kl_decrease is None
    if kw["required"] is not None:
        R = kw["required"]
        assert got.active[R].all() and (got.removal_round[R] == -1).all() and np.isnan(got.kl_increase[R]).all()
    # 2. off the candidate set: exactly 0.0, inactive, never tried
    assert (got.exposures[~C] == 0.0).all() and not got.active[~C].any() and (got.dense_exposures[~C] == 0.0).all()
    assert np.isnan(got.kl_increase[~C]).all() and (got.removal_round[~C] == -1).all()
    assert np.array_equal(got.exposures == 0.0, ~got.active)
    assert np.array_equal(np.isnan(got.kl_increase[rows]), np.isnan(a.kl_increase[rows]))
    # 3. phase 0 is refit_exposures on the sub-catalogue, bit for bit
    H, err, nit, conv = sub_refit(X, W, C, FIXED)
    assert np.array_equal(got.dense_exposures, H) and np.array_equal(got.dense_errors, err)
    assert np.array_equal(got.dense_n_iterations, nit) and np.array_equal(got.dense_converged, conv)
    # 4. values
    dH, dF = mref.deviations(got, ld, scale, rows)
    print(f"masks {case}: isolated {ok.sum()} of {ok.size}, trials {got.n_trials.min()}..{got.n_trials.max()}, threshold margin {margin:.3g}, "
          f"u margin {umargin:.3g}, host spread H {h_spread:.3g} f {f_spread:.3g}, device H {dH:.3g} f {dF:.3g}")
    assert h_spread <= mref.H_SPREAD and f_spread <= mref.F_SPREAD
    assert dH <= 16 * mref.H_SPREAD
    assert dF <= 16 * mref.F_SPREAD


# Sub-catalogue equivalence on the device, shared (K,) sets.  "prefix" (K = 40, C = 0..32): K and |C| give the same KT = 3 and
# every candidate keeps its position, so every product sees the same operands in the same places -- bit for bit.  "word"
# (K = 33, |C| = 32: KT 3 against 2) and "shared" (K = 16, a random subset: other positions) run the same sums with the
# signatures in other slots of the P^T product, so their values are held to the value bound.
@pytest.mark.parametrize("case,exact", [(c, c[4] == "prefix") for c in mref.CASES if c[4] in ("prefix", "word", "shared") and c[1] > 1], ids=str)
def test_a_masked_call_is_the_call_on_the_sub_catalogue(case, exact):
    X, W, kw, runs, (ok, _, _) = mref.case_replicas(*case)
    rows = np.flatnonzero(ok)
    idx = np.flatnonzero(kw["candidates"])
    more = dict(max_kl_increase=kw["max_kl_increase"], readd=kw["readd"], **FIXED)
    got = sal.assign_signatures(X, W, candidates=kw["candidates"], **more)
    sub = sal.assign_signatures(X, W[idx], **more)
    for name in ("active", "removal_round") + (("readd_round",) if kw["readd"] else ()):
        assert np.array_equal(getattr(got, name)[np.ix_(rows, idx)], getattr(sub, name)[rows]), name
    for name in ("n_trials", "n_iterations"):
        assert np.array_equal(getattr(got, name)[rows], getattr(sub, name)[rows]), name
    if exact:
        for name in ("exposures", "kl_increase", "dense_exposures"):
            assert np.array_equal(getattr(got, name)[:, idx], getattr(sub, name), equal_nan=True), name
        for name in ("reconstruction_errors", "dense_errors", "converged"):
            assert np.array_equal(getattr(got, name), getattr(sub, name)), name
    else:
        ld = runs[2]
        scale = mref.row_scale(X, W, ld.exposures)
        wide = lambda r: type("Run", (), dict(exposures=scatter(r.exposures, idx, W.shape[0], 0.0), reconstruction_errors=r.reconstruction_errors,  # noqa: E731
                                              kl_increase=scatter(r.kl_increase, idx, W.shape[0], np.nan),
                                              kl_decrease=None if r.kl_decrease is None else scatter(r.kl_decrease, idx, W.shape[0], np.nan)))
        dH, dF = mref.deviations(wide(sub), ld, scale, rows)
        print(f"sub-catalogue {case}: device H {dH:.3g} f {dF:.3g}")
        assert dH <= 16 * mref.H_SPREAD and dF <= 16 * mref.F_SPREAD


def scatter(a, idx, K, fill):
    out = np.full((a.shape[0], K), fill, dtype=a.dtype)
    out[:, idx] = a
    return out


def test_planted_catalogue_with_the_re_addition_pass():
    """The committed planted case (tests/test_assign_masks_host.py: seed 94, the seed in 0..99 whose re-addition pass accepts
    two signatures; no seed in that range has a planted signature to restore), at the 200 fixed steps of the search; the
    replica's decisions are isolated in 12 of 12 rows."""
    X, W, planted = aref.planted_catalogue(seed=mref.PLANTED_SEED)
    solve = dict(min_iterations=200, max_iterations=200, conv_test_freq=10)
    runs = mref.three_runs(X, W, solve=solve, readd=True)
    ok, margin, umargin = mref.isolation(runs, 1.92)
    got = sal.assign_signatures(X, W, readd=True, **solve)
    print(f"planted with re-addition, T = 200: isolated rows {ok.sum()} of 12, threshold margin {margin:.3g}, u margin {umargin:.3g}, "
          f"re-added {(got.readd_round >= 0).sum()}")
    assert (~ok).sum() <= 1
    assert (got.active | ~planted).all()
    for name in ("active", "removal_round", "readd_round", "n_trials"):
        assert np.array_equal(getattr(got, name)[ok], getattr(runs[0], name)[ok]), name
    assert (got.readd_round[ok] >= 0).sum() == 2 and np.array_equal(got.exposures == 0.0, ~got.active)


def test_an_empty_pool_makes_the_pass_a_no_op():
    X, W = ref.poisson_catalogue(40, 17, seed=12, zero_heavy=2)
    C = mref.case_sets(40, 17, 3, "random")[0]
    for kw in (dict(max_kl_increase=-1e300), dict(candidates=C, required=C), dict(candidates=mref.case_sets(40, 17, 4, "single")[0])):
        off, on = sal.assign_signatures(X, W, readd=False, **kw, **FIXED), sal.assign_signatures(X, W, readd=True, **kw, **FIXED)
        same(on, off)
        assert (on.readd_round == -1).all() and np.isnan(on.kl_decrease).all()
        assert np.array_equal(on.active, np.ones((40, 17), dtype=bool) if "candidates" not in kw else on.candidates)


# ---- independence, with sets and the re-addition pass on

def sets_for(N, K, seed):
    C, R = mref.case_sets(N, K, seed, "required")
    return dict(candidates=C, required=R, readd=True, max_kl_increase=0.1)


@pytest.mark.parametrize("N", [1, 15, 16, 17])
def test_row_subsets_give_the_same_bits(N):
    X, W = ref.poisson_catalogue(100, 33, seed=4, zero_heavy=2)
    sets = sets_for(100, 33, 2)
    full = sal.assign_signatures(X, W, **sets, **CONVERGING)
    assert 1 < np.unique(full.n_iterations).size and 1 < np.unique(full.n_trials).size and (full.kl_decrease == full.kl_decrease).any()
    rows = np.random.default_rng(N).permutation(100)[:N]
    part = sal.assign_signatures(X[rows], W, **dict(sets, candidates=sets["candidates"][rows], required=sets["required"][rows]), **CONVERGING)
    same(part, full, NAMES + READD, rows)


def test_resamples_and_chunks_give_the_same_bits():
    N, K = 37, 33
    X, W = ref.poisson_catalogue(N, K, seed=11, zero_heavy=2)
    sets = sets_for(N, K, 5)
    kw = dict(min_iterations=20, max_iterations=100, conv_test_freq=10, tol=1e-5)
    qs = (0.025, 0.5, 0.975)
    call = lambda R, **more: sal.assign_signatures(X, W, n_resamples=R, resample_seed=5, quantiles=qs, keep_resamples=True, **sets, **kw, **more)  # noqa: E731
    r8, r4 = call(8), call(4)
    small = call(8, chunk_bytes=3 * N * 96 * 8)
    assert r8.timings["n_chunks"] == 1 and small.timings["n_chunks"] == 3
    same(small, r8, NAMES + READD + RESAMPLED)
    same(r4, r8, NAMES + READD)
    assert np.array_equal(r4.exposures_resampled, r8.exposures_resampled[:4])
    Hr = r8.exposures_resampled
    assert (Hr[:, ~sets["candidates"]] == 0.0).all() and (Hr[:, sets["required"]] > 0.0).all()  # a resample has its sample's sets
    assert np.array_equal(r8.selection_frequency, (Hr > 0).mean(axis=0))
    drawn = sal.resample_counts(X, 8, 5)
    for r in (0, 7):  # a resample's problems are those of a call on the drawn matrix with the same sets
        assert np.array_equal(Hr[r], sal.assign_signatures(drawn[r], W, **sets, **kw).exposures), r
