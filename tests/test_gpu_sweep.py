"""KLNMFSweep on the MI355X: every member bit for bit the single fit of the tutorial's loop.

Member (K, s) is compared with ``KLNMF(K, ..., objective_in_step=False).fit(adata.copy(), given, init_kwargs | {"seed": s})``
by ``np.array_equal`` / list equality: signatures, exposures, objective history, iteration count and per-sample
reconstruction errors (``csrc/salnmf_batch.h``: the step calls the same body as the single-model small-cohort kernel, the
objective and per-sample passes call the same body as the forward kernel, with the engine's grid)."""
import os

import numpy as np
import pytest

import salamander_amd as sal
from conftest import GOLDEN, read_counts
from oracle import klnmf_oracle as orc

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def pcawg():
    return sal.AnnData(read_counts(os.path.join(GOLDEN, "pcawg_breast_sbs.csv")).T)


def single(adata, K, settings, init_kwargs=None, given=None):
    m = sal.models.KLNMF(K, objective_in_step=False, **settings)
    m.fit(adata.copy(), given, init_kwargs)
    m.compute_reconstruction_errors()
    m._engine.close()
    return m


def assert_same(got, ref):
    assert got.n_signatures == ref.n_signatures
    assert got.n_iterations_ == ref.n_iterations_, (got.n_signatures, got.n_iterations_, ref.n_iterations_)
    assert got.history["objective_function"] == ref.history["objective_function"], got.n_signatures
    assert np.array_equal(got.asignatures.X, ref.asignatures.X), got.n_signatures
    assert np.array_equal(got.adata.obsm["exposures"], ref.adata.obsm["exposures"]), got.n_signatures
    assert np.array_equal(np.asarray(got.adata.obs["reconstruction_error"]), np.asarray(ref.adata.obs["reconstruction_error"]))
    assert got.reconstruction_error == ref.reconstruction_error


def test_the_tutorials_sweep(pcawg):
    """tutorial.ipynb section 1.6: K = 1..9, default nndsvd initialisation and settings."""
    X_before = np.array(pcawg.X, copy=True)
    s = sal.models.KLNMFSweep(range(1, 10))
    models = s.fit(pcawg)
    assert s.batched_.all()
    assert np.array_equal(pcawg.X, X_before) and "exposures" not in pcawg.obsm and "reconstruction_error" not in pcawg.obs
    refs = [single(pcawg, K, {}) for K in range(1, 10)]
    for got, ref in zip(models, refs):
        assert_same(got, ref)
    assert np.array_equal(s.reconstruction_errors_[:, 0], [r.reconstruction_error for r in refs])


def test_random_inits_seeds_and_a_shrinking_active_set(pcawg):
    settings = dict(init_method="random", min_iterations=20, max_iterations=137, conv_test_freq=10, tol=1e-4)
    Ks, seeds = [1, 2, 5, 8, 13, 16], [0, 1, 2]
    s = sal.models.KLNMFSweep(Ks, seeds=seeds, **settings)
    models = s.fit(pcawg)
    assert s.batched_.all() and len(models) == 18
    iters = [m.n_iterations_ for m in models]
    assert len(set(iters)) >= 3 and 137 in iters, iters  # converged at different tests, and one stopped by the cap
    refs = [single(pcawg, K, settings, {"seed": sd}) for K in Ks for sd in seeds]
    for got, ref in zip(models, refs):
        assert_same(got, ref)
    assert s.reconstruction_errors_.shape == (6, 3)


def test_given_signatures_and_the_all_given_fallback(pcawg):
    settings = dict(min_iterations=30, max_iterations=200, tol=1e-6)
    fitted = single(pcawg, 3, settings)
    given = sal.AnnData(fitted.asignatures.X[:2].copy())
    given.var_names = pcawg.var_names
    gp = {"asignatures": given}
    s = sal.models.KLNMFSweep(range(2, 7), **settings)
    models = s.fit(pcawg, given_parameters=gp)
    assert list(s.batched_) == [False, True, True, True, True]
    for got, K in zip(models, range(2, 7)):
        assert_same(got, single(pcawg, K, settings, given=gp))
        assert np.array_equal(got.asignatures.X[:2], fitted.asignatures.X[:2])


@pytest.mark.parametrize("N,V", [(16, 96), (100, 83), (257, 96), (1024, 96), (1100, 96)])
def test_cohort_shapes_through_every_workgroup_variant(N, V):
    """N = 16 / 100 / 257 / 1024: one to four groups of waves, one and several tiles per wave; N = 1100 and K = 20 are
    outside the batched kernel's reach and take KLNMF.fit."""
    X, _, _ = orc.synthetic_problem(V, N, 4, seed=N + V)
    adata = sal.AnnData(X)
    settings = dict(init_method="random", min_iterations=20, max_iterations=64, tol=1e-5)
    Ks = [1, 6, 11, 20]
    s = sal.models.KLNMFSweep(Ks, seeds=[3], **settings)
    models = s.fit(adata)
    assert list(s.batched_) == [N <= 1024 and K <= 16 for K in Ks]
    for got, K in zip(models, Ks):
        assert_same(got, single(adata, K, settings, {"seed": 3}))


def test_order_and_the_callers_data(pcawg):
    ad = pcawg.copy()
    before = np.array(ad.X, copy=True)
    s = sal.models.KLNMFSweep([3, 1, 2], seeds=[5, 4], init_method="random", min_iterations=10, max_iterations=30)
    models = s.fit(ad)
    assert [m.n_signatures for m in models] == [3, 3, 1, 1, 2, 2]  # K-major, seed-minor
    assert np.array_equal(ad.X, before) and "exposures" not in ad.obsm and "reconstruction_error" not in ad.obs
    assert all(m.adata is not ad and m.adata.X is not ad.X for m in models)
