"""KLNMFSweep's host logic on CPU: validation, the member contract and the cadence of the batched loop.

The device is replaced by oracle-backed fakes (tests only): ``FakeEngine`` for single fits and per-member
initialisation, ``FakeBatchEngine`` for the batch.  Both run the same oracle arithmetic, so every member of a sweep must
equal the single ``KLNMF.fit`` bit for bit here; on the device the same is checked by tests/test_gpu_sweep.py."""

import os

import numpy as np
import pytest

import salamander_amd as sal
from _fake_batch_engine import FakeBatchEngine
from _fake_engine import FakeEngine
from conftest import REF_FIX, read_counts
from salamander_amd.models import signature_nmf, sweep


@pytest.fixture
def fakes(monkeypatch):
    monkeypatch.setattr(signature_nmf, "Engine", FakeEngine)
    monkeypatch.setattr(sweep, "BatchEngine", FakeBatchEngine)
    FakeBatchEngine.instances = []
    return FakeBatchEngine


@pytest.fixture
def adata():
    return sal.AnnData(read_counts(os.path.join(REF_FIX, "klnmf", "counts.csv")).T)


def single(adata, K, settings, init_kwargs=None, given=None):
    m = sal.models.KLNMF(K, objective_in_step=False, **settings)
    m.fit(adata.copy(), given, init_kwargs)
    m.compute_reconstruction_errors()
    return m


def assert_same(a, b):
    assert np.array_equal(a.asignatures.X, b.asignatures.X)
    assert np.array_equal(a.adata.obsm["exposures"], b.adata.obsm["exposures"])
    assert a.history["objective_function"] == b.history["objective_function"]
    assert a.n_iterations_ == b.n_iterations_
    assert np.array_equal(np.asarray(a.adata.obs["reconstruction_error"]), np.asarray(b.adata.obs["reconstruction_error"]))


def test_validation_errors(fakes, adata):
    for bad in ([], [0, 2], [-1], [2.5]):
        with pytest.raises(ValueError):
            sal.models.KLNMFSweep(bad)
    with pytest.raises(ValueError):
        sal.models.KLNMFSweep([2], distributed=True)
    s = sal.models.KLNMFSweep([2, 3], max_iterations=20)
    with pytest.raises(ValueError, match="weighted"):
        s.fit(adata, fitting_kwargs={"weights_kl": np.ones(adata.n_obs)})
    given = sal.AnnData(np.full((3, adata.n_vars), 1.0 / adata.n_vars))
    given.var_names = adata.var_names
    with pytest.raises(ValueError, match="exceeds"):
        s.fit(adata, given_parameters={"asignatures": given})
    with pytest.raises(TypeError):
        s.fit(np.ones((4, 4)))


SETTINGS = dict(min_iterations=30, max_iterations=97, conv_test_freq=10, tol=1e-4)


@pytest.mark.parametrize("init_method,seeds", [("nndsvd", None), ("random", [0, 1])])
def test_members_equal_single_fits(fakes, adata, init_method, seeds):
    settings = dict(SETTINGS, init_method=init_method)
    X_before = np.array(adata.X, copy=True)
    s = sal.models.KLNMFSweep([1, 2, 4], seeds=seeds, **settings)
    models = s.fit(adata)
    assert np.array_equal(adata.X, X_before) and "exposures" not in adata.obsm  # the caller's data is untouched
    assert s.batched_.all() and len(models) == 3 * max(1, len(seeds or []))
    np.random.seed(1234)  # (the random method with a seed reseeds the legacy RNG itself; same order as the sweep)
    want = [single(adata, K, settings, None if seed is None else {"seed": seed}) for K in (1, 2, 4) for seed in (seeds or [None])]
    for got, ref in zip(models, want):
        assert got.n_signatures == ref.n_signatures
        assert_same(got, ref)
    assert s.reconstruction_errors_.shape == (3, max(1, len(seeds or [])))
    assert np.array_equal(s.reconstruction_errors_.ravel(), [m.reconstruction_error for m in want])
    assert all(m._engine is None for m in models) and FakeBatchEngine.instances[-1].closed


def test_no_read_before_min_iterations_and_steps_to_each_stop(fakes, adata):
    s = sal.models.KLNMFSweep([1, 2, 3], min_iterations=50, max_iterations=57, conv_test_freq=10, tol=0.0)
    s.fit(adata)
    b = FakeBatchEngine.instances[-1]
    # objectives at 0, 10, ..., 50; nothing is read before iteration 50, whose test is the first that can stop anyone
    assert [q[0] for q in b.queued] == [0, 1, 2, 3, 4, 5]
    assert b.reads == [(0, 6)]
    # every step call runs exactly to the next test or the cap (57 is not a multiple of 10)
    assert [c[0] for c in b.step_calls] == [10, 10, 10, 10, 10, 7]
    assert all(m.n_iterations_ == 57 for m in s.models_)
    assert s.member_steps_ == 3 * 57


def test_converged_members_leave_the_step_calls(fakes, adata):
    settings = dict(min_iterations=20, max_iterations=200, conv_test_freq=10, tol=3e-3)
    s = sal.models.KLNMFSweep([1, 2, 3, 4], **settings)
    models = s.fit(adata)
    b = FakeBatchEngine.instances[-1]
    iters = {m.n_iterations_ for m in models}
    assert len(iters) >= 2, iters  # the members stop at different tests
    for n_steps, members in b.step_calls:
        assert n_steps == 10
    done = 0
    for n_steps, members in b.step_calls:
        done += n_steps
        # a member is stepped only while it has not stopped
        assert all(models[m].n_iterations_ >= done for m in members)
        assert sorted(members) == [m for m in range(4) if models[m].n_iterations_ >= done]
    for got, K in zip(models, (1, 2, 3, 4)):
        assert_same(got, single(adata, K, settings))


def test_fallback_members_and_max_iterations_edge_cases(fakes, adata):
    given_src = single(adata, 2, dict(SETTINGS))
    given = sal.AnnData(given_src.asignatures.X.copy())
    given.var_names = adata.var_names
    gp = {"asignatures": given}
    s = sal.models.KLNMFSweep([2, 3], **SETTINGS)
    models = s.fit(adata, given_parameters=gp)
    assert list(s.batched_) == [False, True]  # K == n_given: all signatures given, the single-engine fit
    for got, K in zip(models, (2, 3)):
        assert_same(got, single(adata, K, SETTINGS, given=gp))
    for cap in (0, -3, 5):
        settings = dict(SETTINGS, max_iterations=cap)
        models = sal.models.KLNMFSweep([1, 3], **settings).fit(adata)
        for got, K in zip(models, (1, 3)):
            assert_same(got, single(adata, K, settings))
