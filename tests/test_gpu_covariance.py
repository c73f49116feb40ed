"""``sal.exposure_covariance`` on the device against the contract in extended precision (tests/_cov_ref.py).

N = 40 samples; K in {1, 3, 16, 17, 64, 96} -- both edges of a tile of 16 signatures and every instantiation of the kernel; V in
{7, 96}; both kinds of information.  The tolerance is not chosen: ``MEASURED`` records, per case, the largest deviation of the four
float64 replicas of the contract from the long-double reference on these very inputs (relative for ``standard_errors``,
``inflation`` and ``information_diag``, absolute for the correlations and the smallest pivot), measured on the CPU by
``tests/test_cov_host.py::test_the_recorded_tolerances_hold``, which fails when a replica exceeds its record.  The device gets 16
times the record -- the project's margin for another summation order on the same arithmetic.
"""

import os
from functools import lru_cache

import numpy as np
import pytest

import _cov_ref as ref
import salamander_amd as sal

pytestmark = pytest.mark.gpu

N = ref.GPU_N
MARGIN = 16
INFORMATION = ("observed", "expected")
# (case, information) -> (relative, absolute): the replicas' largest deviation from the reference, rounded up to two digits
MEASURED = {
    (1, 7, "observed"): (3.4e-16, 0.0),
    (1, 7, "expected"): (2.4e-16, 0.0),
    (1, 96, "observed"): (3.1e-15, 0.0),
    (1, 96, "expected"): (1.1e-15, 0.0),
    (3, 7, "observed"): (5.3e-16, 2.5e-16),
    (3, 7, "expected"): (4.6e-16, 2.4e-16),
    (3, 96, "observed"): (1.1e-15, 1.7e-16),
    (3, 96, "expected"): (1.1e-15, 2e-16),
    (16, 7, "observed"): (1.7e-13, 4.8e-14),
    (16, 7, "expected"): (3.2e-13, 7.3e-14),
    (16, 96, "observed"): (1.6e-15, 3.1e-16),
    (16, 96, "expected"): (1.7e-15, 4e-16),
    (17, 7, "observed"): (1.2e-13, 3.6e-14),
    (17, 7, "expected"): (1.8e-13, 5.8e-14),
    (17, 96, "observed"): (2.1e-15, 7.1e-16),
    (17, 96, "expected"): (1.6e-15, 4.3e-16),
    (64, 7, "observed"): (3e-13, 5.9e-14),
    (64, 7, "expected"): (2e-13, 3.7e-14),
    (64, 96, "observed"): (1.9e-15, 6.8e-16),
    (64, 96, "expected"): (1.7e-15, 7.1e-16),
    (96, 7, "observed"): (2.1e-13, 1.7e-14),
    (96, 7, "expected"): (5.4e-14, 1.2e-14),
    (96, 96, "observed"): (2.3e-15, 8.6e-16),
    (96, 96, "expected"): (2.1e-15, 6.7e-16),
    ("confounded", "observed"): (1.4e-12, 8.4e-14),
    ("confounded", "expected"): (3.2e-12, 1.6e-13),
}
PER_SIGNATURE = ("standard_errors", "inflation", "information_diag", "max_abs_correlation")


@lru_cache(maxsize=None)
def inputs(case):
    """-> (X, W, H, active or None) of a case: (K, V) or a name"""
    if case == "confounded":
        return (*ref.confounded_case(N, 16, 96), None)
    if case == "duplicate":
        return (*ref.duplicate_case(N, 16, 96), None)
    return ref.gpu_case(*case)


@lru_cache(maxsize=None)
def reference(case, information):
    X, W, H, A = inputs(case)
    r = ref.reference(X, W, H, A, information)
    # `singular` must not hinge on rounding: the reference's smallest pivot is far from the threshold, or exactly 0
    piv = np.asarray(r.min_pivot_value, dtype=np.float64)[r.n_active > 0]
    assert ((piv >= 1e-6) | (piv == 0.0)).all(), piv.min()
    assert np.array_equal(r.singular[r.n_active > 0], piv == 0.0)
    return r


def check(res, r, measured, what):
    """The device's result `res` against the reference `r` at 16 times the replicas' recorded deviation"""
    rel_tol, abs_tol = MARGIN * measured[0], MARGIN * measured[1]
    assert np.array_equal(res.singular, r.singular) and np.array_equal(res.n_active, r.n_active)
    assert res.most_confounded.dtype == np.int32 and res.n_active.dtype == np.int32 and res.singular.dtype == bool
    assert (res.min_pivot_value[res.singular] <= res.min_pivot).all()
    rel, absolute = ref.deviation(res, r)  # (asserts that the NaN patterns agree)
    print(f"{what}: relative {rel:.3g} (allowed {rel_tol:.3g}), absolute {absolute:.3g} (allowed {abs_tol:.3g}), "
          f"{int(r.singular.sum())} singular, inflation up to {np.nanmax(np.asarray(r.inflation, dtype=float), initial=0.0):.3g}")
    assert rel <= rel_tol and absolute <= abs_tol
    # the partner: the reference's wherever its two largest |corr| of the row are more than 10 tolerances apart
    defined = r.most_confounded >= 0
    assert np.array_equal(res.most_confounded >= 0, defined)
    clear = defined & (np.asarray(r.gap, dtype=np.float64) > 10.0 * abs_tol)
    if defined.any():
        assert (defined & ~clear).sum() <= 0.05 * defined.sum()
    assert np.array_equal(res.most_confounded[clear], r.most_confounded[clear])
    assert (res.most_confounded[~defined] == -1).all()


@pytest.mark.parametrize("information", INFORMATION)
@pytest.mark.parametrize("K,V", ref.GPU_SHAPES)
def test_device_against_the_extended_reference(K, V, information):
    X, W, H, A = inputs((K, V))
    res = sal.exposure_covariance(X, W, H, active=A, information=information, return_correlation=True)
    check(res, reference((K, V), information), MEASURED[(K, V, information)], f"K={K} V={V} {information}")
    assert res.correlation.shape == (N, K, K) and res.information == information
    assert res.timings["n_chunks"] == 1 and res.timings["information_kernel_ms"] > 0.0


@pytest.mark.parametrize("information", INFORMATION)
def test_confounded_signatures_name_each_other(information):
    X, W, H, A = inputs("confounded")
    res = sal.exposure_covariance(X, W, H, information=information, return_correlation=True)
    r = reference("confounded", information)
    check(res, r, MEASURED[("confounded", information)], f"confounded {information}")
    # signature 2 is 0.98 of signature 0 (and 0.02 of signature 1, which carries no exposure and is inactive)
    for got in (res, r):
        assert (got.most_confounded[:, 2] == 0).all() and (got.most_confounded[:, 0] == 2).all()
    assert (res.max_abs_correlation[:, 2] > 0.9).all() and (res.inflation[:, 2] > 10.0).all()
    assert np.isnan(res.standard_errors[:, 1]).all() and (res.n_active == 15).all() and not res.singular.any()


def test_a_duplicated_signature_is_singular():
    X, W, H, A = inputs("duplicate")
    r = reference("duplicate", "observed")
    assert r.singular.all() and (np.asarray(r.min_pivot_value, dtype=float) == 0.0).all()
    for information in INFORMATION:
        res = sal.exposure_covariance(X, W, H, information=information, return_correlation=True)
        assert res.singular.all() and (res.n_active == 16).all() and (res.min_pivot_value <= 1e-10).all()
        for name in PER_SIGNATURE:
            assert np.isnan(getattr(res, name)).all(), name
        assert (res.most_confounded == -1).all() and np.isnan(res.correlation).all()
    # without the copy the same samples are regular
    A = np.ones(16, dtype=bool)
    A[2] = False
    res = sal.exposure_covariance(X, W, H, active=A)
    want = ref.reference(X, W, H, A)
    assert not res.singular.any() and not want.singular.any() and (res.n_active == 15).all()
    assert np.isnan(res.inflation[:, 2]).all() and np.isfinite(np.delete(res.inflation, 2, axis=1)).all()


def test_inactive_entries_and_samples_without_an_active_signature():
    K, V = 16, 96
    X, W, H, A = inputs((K, V))
    res = sal.exposure_covariance(X, W, H, return_correlation=True)  # the default set is exposures > 0
    assert np.array_equal(res.active, A) and np.array_equal(res.active, H > 0.0)
    r = reference((K, V), "observed")
    check(res, r, MEASURED[(K, V, "observed")], "default active set")
    assert res.n_active.tolist() == [16] * 5 + [8, 8, 0] + [16] * 32
    for name in PER_SIGNATURE:
        got = getattr(res, name)
        assert np.array_equal(np.isnan(got), ~A), name  # NaN exactly on the inactive entries: nothing here is singular
    assert np.array_equal(res.most_confounded == -1, ~A)
    assert not res.singular[7] and np.isnan(res.min_pivot_value[7]) and np.isnan(res.correlation[7]).all()
    # an explicit set on a sample with exposure everywhere
    A2 = A.copy()
    A2[0, ::2] = False
    res2 = sal.exposure_covariance(X, W, H, active=A2)
    want = ref.reference(X, W, H, A2)
    rel, absolute = ref.deviation(res2, want)
    assert rel <= MARGIN * MEASURED[(K, V, "observed")][0] and absolute <= MARGIN * MEASURED[(K, V, "observed")][1]
    assert res2.n_active[0] == 8 and np.array_equal(np.isnan(res2.standard_errors[0]), ~A2[0])
    # the others never met sample 0
    for name in PER_SIGNATURE + ("most_confounded", "min_pivot_value"):
        assert np.array_equal(getattr(res2, name)[1:], getattr(res, name)[1:], equal_nan=True), name


def same(a, b, rows_a=slice(None), rows_b=slice(None), correlation=True):
    for name in PER_SIGNATURE + ("most_confounded", "min_pivot_value", "singular", "n_active") + (("correlation",) if correlation else ()):
        assert np.array_equal(getattr(a, name)[rows_a], getattr(b, name)[rows_b], equal_nan=True), name


@pytest.mark.parametrize("K,V", [(17, 96), (64, 7)])
def test_a_samples_results_are_its_own(K, V):
    X, W, H, A = inputs((K, V))
    full = sal.exposure_covariance(X, W, H, active=A, return_correlation=True)
    rows = np.array([3, 0, 17, 39, 6])
    sub = sal.exposure_covariance(X[rows], W, H[rows], active=A[rows], return_correlation=True)
    same(sub, full, rows_b=rows)
    perm = np.random.default_rng(0).permutation(N)
    shuffled = sal.exposure_covariance(X[perm], W, H[perm], active=A[perm], return_correlation=True)
    same(shuffled, full, rows_b=perm)
    one = sal.exposure_covariance(X[11:12], W, H[11:12], active=A[11:12], return_correlation=True)
    same(one, full, rows_b=slice(11, 12))
    # seven samples per chunk of the correlation buffer: six launches
    chunked = sal.exposure_covariance(X, W, H, active=A, return_correlation=True, chunk_bytes=7 * K * K * 8)
    assert chunked.timings["n_chunks"] == 6 and full.timings["n_chunks"] == 1
    same(chunked, full)
    tiny = sal.exposure_covariance(X, W, H, active=A, return_correlation=True, chunk_bytes=1)
    assert tiny.timings["n_chunks"] == N
    same(tiny, full)
    quiet = sal.exposure_covariance(X, W, H, active=A, chunk_bytes=1)
    assert quiet.correlation is None and quiet.timings["n_chunks"] == 1
    same(quiet, full, correlation=False)
    # the correlation matrix: symmetric bit for bit, a unit diagonal on the active set of a regular sample, NaN elsewhere
    C = full.correlation
    assert np.array_equal(C, C.transpose(0, 2, 1), equal_nan=True)
    live = A & ~full.singular[:, None]
    assert np.array_equal(np.isnan(C), ~(live[:, :, None] & live[:, None, :]))
    assert (np.diagonal(C, axis1=1, axis2=2)[live] == 1.0).all()
    off = np.where(np.eye(K, dtype=bool)[None] | np.isnan(C), -1.0, np.abs(C))
    partner = full.most_confounded >= 0
    assert np.array_equal(off.argmax(axis=2)[partner], full.most_confounded[partner])
    assert np.array_equal(off.max(axis=2)[partner], full.max_abs_correlation[partner])


def test_composition_with_the_refit_and_the_assignment():
    X, W, _ = ref.poisson_case(N, 5, 96, seed=3)
    fit = sal.refit_exposures(X, W)
    a = sal.exposure_covariance(X, W)
    b = sal.exposure_covariance(X, W, fit.exposures)
    assert np.array_equal(a.exposures, fit.exposures) and (a.n_active == 5).all()
    same(a, b, correlation=False)
    assert a.timings["refit_s"] > 0.0 and b.timings["refit_s"] == 0.0
    sparse = sal.assign_signatures(X, W)
    c = sal.exposure_covariance(X, W, sparse.exposures)
    support = sparse.exposures > 0.0
    assert np.array_equal(c.n_active, support.sum(axis=1)) and np.array_equal(c.active, support) and not support.all()
    assert np.array_equal(np.isnan(c.standard_errors), ~support | c.singular[:, None])


def test_pcawg_breast_against_sweep_signatures():
    import pandas as pd

    path = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "pcawg_breast_sbs.csv")
    counts = pd.read_csv(path, index_col=0).T  # samples x 96
    adata = sal.AnnData(counts.values.astype(np.float64))
    adata.var_names = list(counts.columns)
    sweep = sal.models.KLNMFSweep(ns_signatures=[4], seeds=[0, 1, 2], stability=True, min_iterations=200, max_iterations=400)
    sweep.fit(adata)
    S = np.asarray(sweep.consensus_signatures_[0])
    X = np.asarray(adata.X, dtype=np.float64)
    H = sal.refit_exposures(X, S, min_iterations=100, max_iterations=2000).exposures
    for information in INFORMATION:
        res = sal.exposure_covariance(adata, S, H, information=information, return_correlation=True)
        r = ref.reference(X, S, H, None, information)
        piv = np.asarray(r.min_pivot_value, dtype=np.float64)
        assert (piv >= 1e-6).all() and not r.singular.any()
        # the same rule: the replicas' deviation from the reference on these inputs, measured here on the host
        check(res, r, ref.measure(X, S, H, None, information, ref=r), f"pcawg {information}")
        assert res.standard_errors.shape == (X.shape[0], 4) and (res.n_active == 4).all()
