"""KLNMFSweep with bootstrap resamples on the MI355X: every member bit for bit the single fit on its own resample.

Member (K, s, r) is compared with ``KLNMF(K, ..., objective_in_step=False).fit(AnnData(resamples_[r]), given,
init_kwargs | {"seed": s})`` by ``np.array_equal`` / list equality, in the style of tests/test_gpu_sweep.py: signatures,
exposures, objective history, iteration count and per-sample reconstruction errors.  The batched kernels read the member's
own X through its entry of the member table and run the unchanged bodies on it (``csrc/salnmf_batch.h``)."""
import os

import numpy as np
import pytest

import _resample_ref as ref
import salamander_amd as sal
from conftest import GOLDEN, read_counts
from oracle import klnmf_oracle as orc

pytestmark = pytest.mark.gpu

EPSILON = 1.1920928955078125e-07


@pytest.fixture(scope="module")
def pcawg():
    return sal.AnnData(read_counts(os.path.join(GOLDEN, "pcawg_breast_sbs.csv")).T)


def single(X, K, settings, init_kwargs=None, given=None):
    m = sal.models.KLNMF(K, objective_in_step=False, **settings)
    m.fit(sal.AnnData(np.array(X, copy=True)), given, init_kwargs)
    m.compute_reconstruction_errors()
    m._engine.close()
    return m


def assert_same(got, ref_model):
    assert got.n_signatures == ref_model.n_signatures
    assert got.n_iterations_ == ref_model.n_iterations_, (got.n_signatures, got.n_iterations_, ref_model.n_iterations_)
    assert got.history["objective_function"] == ref_model.history["objective_function"], got.n_signatures
    assert np.array_equal(got.asignatures.X, ref_model.asignatures.X), got.n_signatures
    assert np.array_equal(got.adata.obsm["exposures"], ref_model.adata.obsm["exposures"]), got.n_signatures
    assert np.array_equal(np.asarray(got.adata.obs["reconstruction_error"]), np.asarray(ref_model.adata.obs["reconstruction_error"]))
    assert got.reconstruction_error == ref_model.reconstruction_error


def check_members(s, models, Ks, seeds, R, settings, given=None):
    """Every member, in K-major, seed-middle, resample-minor order."""
    members = [(K, sd, r) for K in Ks for sd in (seeds or [None]) for r in range(R)]
    assert len(models) == len(members) and list(s.resample_of_) == [r for _, _, r in members]
    for got, (K, sd, r) in zip(models, members):
        assert_same(got, single(s.resamples_[r], K, settings, None if sd is None else {"seed": sd}, given))
        assert np.array_equal(got.adata.X, np.maximum(s.resamples_[r], EPSILON))
    assert s.reconstruction_errors_.shape == (len(Ks), max(1, len(seeds or [])), R)
    assert np.array_equal(s.reconstruction_errors_.reshape(-1), [m.reconstruction_error for m in models])


def test_the_tutorials_sweep_on_three_resamples(pcawg):
    """K = 1..9, default nndsvd initialisation and settings, R = 3."""
    X_before = np.array(pcawg.X, copy=True)
    s = sal.models.KLNMFSweep(range(1, 10), n_resamples=3, resample_seed=2024)
    models = s.fit(pcawg)
    assert s.batched_.all()
    assert np.array_equal(pcawg.X, X_before) and "exposures" not in pcawg.obsm and "reconstruction_error" not in pcawg.obs
    assert np.array_equal(s.resamples_, ref.resample_counts(X_before, 3, 2024))
    assert all(list(m.adata.obs_names) == list(pcawg.obs_names) and list(m.adata.var_names) == list(pcawg.var_names) for m in models)
    check_members(s, models, range(1, 10), None, 3, {})
    assert len({m.reconstruction_error for m in models[:3]}) == 3  # (three different matrices)


def test_random_inits_seeds_and_a_shrinking_active_set(pcawg):
    settings = dict(init_method="random", min_iterations=20, max_iterations=137, conv_test_freq=10, tol=1e-4)
    Ks, seeds, R = [1, 2, 5, 8, 13, 16], [0, 1], 2
    s = sal.models.KLNMFSweep(Ks, seeds=seeds, n_resamples=R, resample_seed=2**40 + 1, **settings)
    models = s.fit(pcawg)
    assert s.batched_.all() and len(models) == 24
    iters = [m.n_iterations_ for m in models]
    assert len(set(iters)) >= 3 and 137 in iters, iters  # converged at different tests, and one stopped by the cap
    check_members(s, models, Ks, seeds, R, settings)


def test_given_signatures_and_a_17_signature_fallback(pcawg):
    settings = dict(min_iterations=30, max_iterations=200, tol=1e-6)
    fitted = single(pcawg.X, 3, settings)
    given = sal.AnnData(fitted.asignatures.X[:2].copy())
    given.var_names = pcawg.var_names
    gp = {"asignatures": given}
    Ks, R = [2, 4, 17], 2
    s = sal.models.KLNMFSweep(Ks, n_resamples=R, resample_seed=7, **settings)
    models = s.fit(pcawg, given_parameters=gp)
    assert list(s.batched_) == [False, False, True, True, False, False]  # (all given; in reach; 17 signatures)
    members = [(K, r) for K in Ks for r in range(R)]
    for got, (K, r) in zip(models, members):
        ref_model = sal.models.KLNMF(K, objective_in_step=False, **settings)
        ad = pcawg.copy()
        ad.X = s.resamples_[r].copy()  # (given signatures are matched to the data by var_names)
        ref_model.fit(ad, gp, None)
        ref_model.compute_reconstruction_errors()
        ref_model._engine.close()
        assert_same(got, ref_model)
        assert np.array_equal(got.asignatures.X[:2], fitted.asignatures.X[:2])
    assert s.reconstruction_errors_.shape == (3, 1, 2)


@pytest.mark.parametrize("N", [40, 300])
def test_other_cohort_sizes(N):
    """40 and 300 samples: other workgroup variants of the batched step (NG = 1, and NG = 4 with several tiles per wave)."""
    rng = np.random.default_rng(N)
    P, _, _ = orc.synthetic_problem(96, N, 4, seed=N)
    X = rng.poisson(P * (2000.0 / P.sum(axis=1, keepdims=True))).astype(float)
    adata = sal.AnnData(X)
    settings = dict(init_method="random", min_iterations=20, max_iterations=64, tol=1e-5)
    Ks, R = [1, 6, 11], 2
    s = sal.models.KLNMFSweep(Ks, seeds=[3], n_resamples=R, resample_seed=N, **settings)
    models = s.fit(adata)
    assert s.batched_.all() and np.array_equal(adata.X, X)
    assert np.array_equal(s.resamples_, ref.resample_counts(X, R, N))
    check_members(s, models, Ks, [3], R, settings)


def test_beyond_the_batch_the_resamples_come_from_the_stand_alone_entry():
    """V = 120 > 96: no batch at all; the members run KLNMF.fit on resamples drawn by sal.resample_counts."""
    rng = np.random.default_rng(1)
    X = rng.poisson(rng.gamma(0.5, 40.0, size=(50, 120))).astype(float)
    settings = dict(init_method="random", min_iterations=10, max_iterations=30)
    s = sal.models.KLNMFSweep([2, 3], seeds=[1], n_resamples=2, resample_seed=9, **settings)
    models = s.fit(sal.AnnData(X))
    assert not s.batched_.any() and np.array_equal(s.resamples_, ref.resample_counts(X, 2, 9))
    check_members(s, models, [2, 3], [1], 2, settings)


def test_without_resamples_a_sweep_is_what_it_was(pcawg):
    settings = dict(init_method="random", min_iterations=10, max_iterations=30)
    s = sal.models.KLNMFSweep([3, 2], seeds=[5, 4], n_resamples=0, **settings)
    models = s.fit(pcawg)
    assert s.reconstruction_errors_.shape == (2, 2) and s.resamples_ is None and list(s.resample_of_) == [-1] * 4
    for got, (K, sd) in zip(models, [(3, 5), (3, 4), (2, 5), (2, 4)]):
        assert_same(got, single(pcawg.X, K, settings, {"seed": sd}))


def test_bad_counts_are_refused_before_the_device(pcawg):
    X = np.array(pcawg.X, dtype=float)
    X[17, 3] += 0.5
    with pytest.raises(ValueError, match="row 17"):
        sal.models.KLNMFSweep([2], n_resamples=2).fit(sal.AnnData(X))
