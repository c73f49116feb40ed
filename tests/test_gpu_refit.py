"""``sal.refit_exposures`` on the device against the host replica (tests/_refit_ref.py), DESIGN.md section 13.

Tolerances are not tuned on the device.  For every case the test itself measures, on the CPU and on the case's own inputs,
how far the float64 replica in two feature orders lies from the longdouble replica; the device -- a third summation order,
the MFMA's -- is one more sample from that distribution and gets 16 x the measured value.  H is compared entry by entry as
|dH| / max(H_ref, EPSILON).  The recorded constants below are 16 x the largest value measured over this file's cases
(host run: fixed-step spread 3.83e-14 at T = 200, K = 96; deviation of the relative change 1.93e-7 at tol = 1e-7, K = 24); each test asserts
that its own measurement stays within the recorded one, so the constants cannot drift from the inputs.
"""

import numpy as np
import pytest

import _refit_ref as ref
import salamander_amd as sal

pytestmark = pytest.mark.gpu

EPS = ref.EPSILON
H_SPREAD = 3.9e-14  # measured 3.83e-14: largest |dH| / max(H_ld, EPS), float64 replica (two feature orders) against longdouble, T = 200, this file's cases
H_TOL = 16 * H_SPREAD
G_RAW = 2.0e-7  # measured 1.93e-7: largest |change - change_ld| / max(change_ld, tol), same replicas, eligible tests up to each problem's stop
# (measured at this file's K <= 24.  It does not hold at every larger K: the same replicas give 1.4e-7 to 5.1e-7 over K = 33..48 and
# 65..80 at N = 32, above the record at most of them; tests/test_gpu_family_edges.py uses K = 35 and K = 80, which hold it)
# (relative to max(change, tol): a change far below tol -- an all-zero row sits at its fixed point, change 0 -- can only flip a test by
# an absolute error of the order of tol)
G = 16 * G_RAW
T = 200


def entry_dev(H, H_ref):
    H_ref = np.asarray(H_ref, dtype=np.longdouble)
    return float((np.abs(H - H_ref) / np.maximum(H_ref, EPS)).max())


def catalogue(N, K, V=96, seed=0):
    """Poisson counts with three zero-heavy rows, one row with a single mutation and one all-zero row."""
    X, W = ref.poisson_catalogue(N, K, V=V, seed=seed, zero_heavy=min(3, N - 1))
    if N > 4:
        X[1] = 0.0
        X[1, V // 2] = 1.0
        X[2] = 0.0
    return X, W


def host_spread(X, W, **kw):
    V = X.shape[1]
    perm = np.random.default_rng(7).permutation(V)
    ld = ref.refit(X, W, dtype=np.longdouble, **kw)
    a = ref.refit(X, W, **kw)
    b = ref.refit(X, W, perm=perm, **kw)
    return ld, max(entry_dev(a.exposures, ld.exposures), entry_dev(b.exposures, ld.exposures))


def schedule_spread(X, W, nit, kw):
    """The longdouble replica forced to the stop schedule `nit`, and the float64 replicas' largest deviation from it."""
    perm = np.random.default_rng(7).permutation(X.shape[1])
    forced = ref.refit(X, W, dtype=np.longdouble, schedule=nit, **kw)
    return forced, max(entry_dev(ref.refit(X, W, schedule=nit, **kw).exposures, forced.exposures),
                       entry_dev(ref.refit(X, W, schedule=nit, perm=perm, **kw).exposures, forced.exposures))


CASES = [(40, 1, 96), (40, 3, 96), (40, 16, 96), (40, 17, 96), (40, 64, 96), (40, 96, 96), (40, 3, 7), (33, 8, 96)]


@pytest.mark.parametrize("N,K,V", CASES)
def test_fixed_steps_entry_by_entry(N, K, V):
    X, W = catalogue(N, K, V, seed=K + V)
    kw = dict(min_iterations=T, max_iterations=T)
    ld, spread = host_spread(X, W, **kw)
    got = sal.refit_exposures(X, W, **kw)
    dev = entry_dev(got.exposures, ld.exposures)
    scale = (np.abs(np.maximum(X, EPS) * np.log(np.maximum(X, EPS) / (ld.exposures @ W).astype(np.float64))) + X + 1.0).sum(axis=1)
    derr = float((np.abs(got.reconstruction_errors - ld.reconstruction_errors.astype(np.float64)) / scale).max())
    print(f"fixed N={N} K={K} V={V}: host spread {spread:.3g} device {dev:.3g} tol {H_TOL:.3g} objective/scale {derr:.3g}")
    assert spread <= H_SPREAD
    assert dev <= H_TOL
    assert np.array_equal(got.n_iterations, np.full(N, T))  # (T is a test iteration: a problem may also pass its test there)
    assert got.exposures.min() >= EPS
    # the objective: terms of size `scale` summed in another order, and H itself within H_TOL
    assert derr <= 96 * 2.0**-52 + 4 * H_TOL


@pytest.mark.parametrize("N,K", [(40, 8), (33, 16), (20, 64)])
def test_fixed_steps_against_the_engine(N, K):
    rng = np.random.default_rng(K)
    X, _ = catalogue(N, K, seed=3)
    W = ref.normalize(rng.dirichlet(np.full(96, 0.15), size=K) + 1e-4)
    assert W.min() > EPS  # (the engine's joint step clips even given signatures at EPSILON: nothing to clip here)
    x = np.maximum(X, EPS)
    e = sal.Engine(N, 96, K)
    e.upload_X(x), e.upload_W(W), e.upload_H(ref.start(x, K))
    e.kl_step(T, K)
    H_engine = e.download_H()
    kl_engine = e.samplewise_kl()
    e.close()
    got = sal.refit_exposures(X, W, min_iterations=T, max_iterations=T)
    dev = entry_dev(got.exposures, H_engine)
    print(f"engine N={N} K={K}: {dev:.3g} tol {H_TOL:.3g}")
    assert dev <= H_TOL
    scale = (np.abs(x * np.log(x / (H_engine @ W))) + x + 1.0).sum(axis=1)
    assert np.all(np.abs(got.reconstruction_errors - kl_engine) <= (96 * 2.0**-52 + 4 * H_TOL) * scale)


@pytest.mark.parametrize("N,K", [(48, 3), (48, 8), (32, 24)])
def test_convergence_of_every_problem(N, K):
    X, W = catalogue(N, K, seed=100 + K)
    kw = dict(min_iterations=500, max_iterations=4000, conv_test_freq=10, tol=1e-7)
    got = sal.refit_exposures(X, W, **kw)
    nit = got.n_iterations.astype(np.int64)
    last = int(nit.max())
    free = {name: ref.refit(X, W, free_run=True, **{**kw, "max_iterations": last}, **extra)
            for name, extra in (("ld", dict(dtype=np.longdouble)), ("a", {}), ("b", dict(perm=np.random.default_rng(7).permutation(96))))}
    ld = free["ld"]
    tests = ld.tests
    eligible = tests >= kw["min_iterations"]
    # g on these inputs: deviation of the float64 replicas' relative change from the longdouble one's, at every eligible
    # test up to the longdouble replica's own stop
    ld_stop = np.array([next((t for t, c in zip(tests[eligible], ld.changes[eligible, p]) if c < kw["tol"]), last) for p in range(N)])
    g_raw = 0.0
    for p in range(N):
        m = eligible & (tests <= ld_stop[p])
        for name in ("a", "b"):
            g_raw = max(g_raw, float((np.abs(free[name].changes[m, p] - ld.changes[m, p]) / np.maximum(ld.changes[m, p], kw["tol"])).max(initial=0.0)))
    print(f"convergence N={N} K={K}: iterations {nit.min()}..{np.median(nit):.0f}..{nit.max()}, g_raw {g_raw:.3g} (recorded {G_RAW:.3g}), capped {int((~got.converged).sum())}")
    assert g_raw <= G_RAW
    for p in range(N):  # every problem, near-ties included
        if got.converged[p]:
            i = int(np.flatnonzero(tests == nit[p])[0])
            assert nit[p] >= kw["min_iterations"] and nit[p] % 10 == 0
            assert ld.changes[i, p] < kw["tol"] * (1 + G), (p, nit[p], ld.changes[i, p])
        else:
            assert nit[p] == kw["max_iterations"]
            i = len(tests)
        earlier = eligible & (np.arange(len(tests)) < i)
        assert np.all(ld.changes[earlier, p] >= kw["tol"] * (1 - G)), (p, nit[p])
    forced, spread = schedule_spread(X, W, nit, kw)
    dev = entry_dev(got.exposures, forced.exposures)
    print(f"   H at the device's schedule: host spread {spread:.3g} device {dev:.3g} tol {16 * spread:.3g}")
    assert dev <= 16 * spread


def test_exact_properties_of_the_resamples():
    X, W = catalogue(37, 5, seed=11)
    kw = dict(min_iterations=50, max_iterations=300, conv_test_freq=10, tol=1e-6)
    qs = (0.025, 0.25, 0.5, 0.9, 0.975)
    r8 = sal.refit_exposures(X, W, n_resamples=8, resample_seed=5, quantiles=qs, keep_resamples=True, **kw)
    r4 = sal.refit_exposures(X, W, n_resamples=4, resample_seed=5, quantiles=qs, keep_resamples=True, **kw)
    again = sal.refit_exposures(X, W, n_resamples=8, resample_seed=5, quantiles=qs, keep_resamples=True, **kw)
    small = sal.refit_exposures(X, W, n_resamples=8, resample_seed=5, quantiles=qs, keep_resamples=True, chunk_bytes=3 * 37 * 96 * 8, **kw)
    assert r8.timings["n_chunks"] == 1 and small.timings["n_chunks"] == 3
    drawn = sal.resample_counts(X, 8, 5)
    for r in range(8):
        one = sal.refit_exposures(drawn[r], W, **kw)
        assert np.array_equal(r8.exposures_resampled[r], one.exposures), r
        assert np.array_equal(r8.n_iterations_resampled[r], one.n_iterations) and np.array_equal(r8.reconstruction_errors_resampled[r], one.reconstruction_errors)
    assert 1 < np.unique(r8.n_iterations_resampled).size  # problems of one tile stop at different tests
    assert np.array_equal(r4.exposures_resampled, r8.exposures_resampled[:4])
    for name in ("exposures", "reconstruction_errors", "n_iterations", "converged", "exposures_resampled", "exposures_mean", "exposures_quantiles",
                 "n_iterations_resampled", "reconstruction_errors_resampled"):
        assert np.array_equal(getattr(again, name), getattr(r8, name)), name
        assert np.array_equal(getattr(small, name), getattr(r8, name)), name
    for res, R in ((r8, 8), (r4, 4)):
        mean, quant = ref.reduce_resamples(res.exposures_resampled, qs)
        assert np.array_equal(res.exposures_mean, mean) and np.array_equal(res.exposures_quantiles, quant)
        for i, q in enumerate(qs):
            assert np.array_equal(res.exposures_quantiles[i], np.quantile(res.exposures_resampled, q, axis=0, method="lower" if q <= 0.5 else "higher"))
    assert sal.refit_exposures(X, W, n_resamples=2, **kw).exposures_resampled is None
    for key in ("resample_s", "refit_s", "reduce_s", "total_s", "refit_kernel_ms"):
        assert r8.timings[key] >= 0.0


def test_many_resamples_sort_and_mean():
    X, W = catalogue(9, 3, V=7, seed=2)
    res = sal.refit_exposures(X, W, n_resamples=301, quantiles=(0.0, 0.025, 0.5, 0.975, 1.0), keep_resamples=True, min_iterations=20, max_iterations=60)
    mean, quant = ref.reduce_resamples(res.exposures_resampled, res.quantiles)
    assert np.array_equal(res.exposures_mean, mean) and np.array_equal(res.exposures_quantiles, quant)
    assert np.array_equal(res.exposures_quantiles[0], res.exposures_resampled.min(axis=0)) and np.array_equal(res.exposures_quantiles[4], res.exposures_resampled.max(axis=0))


@pytest.mark.parametrize("N", [1, 15, 16, 17, 1000])
def test_row_subsets_give_the_same_bits(N):
    X, W = ref.poisson_catalogue(1000, 6, seed=4, zero_heavy=5)
    kw = dict(min_iterations=30, max_iterations=200, conv_test_freq=10, tol=1e-5)
    full = sal.refit_exposures(X, W, **kw)
    rows = np.random.default_rng(N).permutation(1000)[:N]
    part = sal.refit_exposures(X[rows], W, **kw)
    for name in ("exposures", "reconstruction_errors", "n_iterations", "converged"):
        assert np.array_equal(getattr(part, name), getattr(full, name)[rows]), name
    if N == 1000:
        assert 1 < np.unique(full.n_iterations).size
        want = ref.refit(X, W, **kw)
        assert np.mean(want.n_iterations == full.n_iterations) > 0.9  # (orientation only: ties may fall either way)


def test_pcawg_consensus_signatures_feed_the_refit():
    import os

    import pandas as pd

    path = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "pcawg_breast_sbs.csv")
    counts = pd.read_csv(path, index_col=0).T  # samples x 96
    adata = sal.AnnData(counts.values.astype(np.float64))
    adata.var_names = list(counts.columns)
    sweep = sal.models.KLNMFSweep(ns_signatures=[3, 4], seeds=[0, 1, 2], stability=True, min_iterations=200, max_iterations=400)
    sweep.fit(adata)
    S = np.asarray(sweep.consensus_signatures_[1])
    X = np.asarray(adata.X, dtype=np.float64)
    kw = dict(min_iterations=100, max_iterations=2000)
    res = sal.refit_exposures(adata, S, n_resamples=20, keep_resamples=True, **kw)
    N, K = X.shape[0], S.shape[0]
    assert K == 4 and res.exposures.shape == (N, K) and res.exposures_quantiles.shape == (3, N, K)
    lo, med, hi = res.exposures_quantiles
    assert np.all(lo <= med) and np.all(med <= hi)
    # a step keeps sum_k h_k = sum_v x_v when W's rows sum to one: to rounding, and up to the EPSILON clips
    assert np.allclose(res.exposures.sum(axis=1), np.maximum(X, EPS).sum(axis=1), rtol=1e-10, atol=2 * K * EPS)
    forced, spread = schedule_spread(X, ref.normalize(S), res.n_iterations.astype(np.int64), kw)
    dev = entry_dev(res.exposures, forced.exposures)
    print(f"pcawg: iterations {res.n_iterations.min()}..{res.n_iterations.max()}, host spread {spread:.3g} device {dev:.3g}")
    assert dev <= 16 * spread
