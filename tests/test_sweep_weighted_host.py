"""KLNMFSweep's penalty axis and shared KL weights on the CPU: members against single fits bit for bit, member order and
shapes, validation and the held-out summaries, on oracle-backed fakes (``_fake_weighted_batch_engine``).

On the MI355X the same comparison runs in tests/test_gpu_sweep_weighted.py."""

import os

import numpy as np
import pytest

import _split_ref as ref
import salamander_amd as sal
from _fake_engine import FakeEngine
from _fake_weighted_batch_engine import FakeWeightedBatchEngine
from conftest import REF_FIX, read_counts
from salamander_amd.models import signature_nmf, sweep

SETTINGS = dict(init_method="random", min_iterations=20, max_iterations=40, conv_test_freq=10, tol=1e-4)


@pytest.fixture
def fakes(monkeypatch):
    monkeypatch.setattr(signature_nmf, "Engine", FakeEngine)
    monkeypatch.setattr(sweep, "Engine", FakeEngine)
    monkeypatch.setattr(sweep, "BatchEngine", FakeWeightedBatchEngine)
    monkeypatch.setattr(sweep, "split_counts", lambda X, F, p, seed, device=0: ref.split_counts(X, F, p, seed))
    FakeWeightedBatchEngine.instances = []
    FakeWeightedBatchEngine.planted = None
    yield FakeWeightedBatchEngine


@pytest.fixture
def adata():
    return sal.AnnData(read_counts(os.path.join(REF_FIX, "klnmf", "counts.csv")).T)


def single(X, K, seed, wkl, lam):
    m = sal.models.KLNMF(K, objective_in_step=False, **SETTINGS)
    m.fit(sal.AnnData(X.copy()), None, {"seed": seed}, {"weights_kl": wkl, "weights_lhalf": lam})
    m.compute_reconstruction_errors()
    return m


def assert_same(got, want):
    assert np.array_equal(got.asignatures.X, want.asignatures.X) and np.array_equal(got.adata.obsm["exposures"], want.adata.obsm["exposures"])
    assert got.history["objective_function"] == want.history["objective_function"] and got.n_iterations_ == want.n_iterations_
    assert np.array_equal(np.asarray(got.adata.obs["reconstruction_error"]), np.asarray(want.adata.obs["reconstruction_error"]))


@pytest.mark.parametrize("with_wkl", [False, True])
@pytest.mark.parametrize("F", [0, 2])
def test_members_equal_single_weighted_fits(fakes, adata, with_wkl, F):
    Ks, lams, seeds = [1, 3], [0.0, 0.5], [0, 1]
    n_obs = adata.X.shape[0]
    wkl = np.random.default_rng(3).uniform(0.5, 2.0, n_obs) if with_wkl else None
    s = sal.models.KLNMFSweep(Ks, seeds=seeds, lhalf_weights=lams, weights_kl=wkl, n_splits=F, split_seed=4, **SETTINGS)
    models = s.fit(adata)
    (engine,) = fakes.instances
    assert s.batched_.all() and engine.weight_calls == list(range(len(models)))
    reps = max(1, F)
    order = [(K, l, sd, f) for K in Ks for l in range(len(lams)) for sd in seeds for f in range(reps)]
    assert [m.n_signatures for m in models] == [o[0] for o in order]
    assert list(s.lhalf_of_) == [o[1] for o in order]
    assert list(s.split_of_) == [o[3] if F else -1 for o in order]
    shape = (len(Ks), len(lams), len(seeds)) + ((F,) if F else ())
    assert s.reconstruction_errors_.shape == shape
    if F:
        assert s.heldout_errors_.shape == shape and s.heldout_mean_.shape == s.heldout_sem_.shape == (len(Ks), len(lams))
        assert np.array_equal(s.heldout_errors_.reshape(-1), [float(np.sum(np.asarray(m.adata.obs["heldout_error"]))) for m in models])
        assert s.suggest_n_signatures_heldout() == s.suggest_penalty_heldout()[0]
    np.random.seed(99)
    for got, (K, l, sd, f), err in zip(models, order, s.reconstruction_errors_.reshape(-1)):
        X = s.train_splits_[f] if F else np.asarray(adata.X)
        want = single(X, K, sd, wkl, lams[l])
        assert_same(got, want)
        assert err == want.reconstruction_error
    # the zero penalty is the penalised closed form, not the unpenalised member
    plain = sal.models.KLNMF(3, objective_in_step=False, **SETTINGS)
    plain.fit(sal.AnnData((s.train_splits_[0] if F else np.asarray(adata.X)).copy()), None, {"seed": 0}, {"weights_kl": wkl})
    zero = models[order.index((3, 0, 0, 0))]
    assert not np.array_equal(zero.adata.obsm["exposures"], plain.adata.obsm["exposures"])


def test_layout_without_the_axis_is_todays(fakes, adata):
    Ks, seeds = [2, 1], [0, 1]
    s = sal.models.KLNMFSweep(Ks, seeds=seeds, **SETTINGS)
    assert s.heldout_mean_.shape == (2,) and s.lhalf_weights is None
    models = s.fit(adata)
    assert [m.n_signatures for m in models] == [2, 2, 1, 1] and list(s.lhalf_of_) == [-1] * 4
    assert s.reconstruction_errors_.shape == (2, 2) and fakes.instances[0].weight_calls == []
    # weights_kl alone: no axis, every member weighted
    w = 2.0
    s = sal.models.KLNMFSweep(Ks, seeds=seeds, weights_kl=w, **SETTINGS)
    models = s.fit(adata)
    assert s.reconstruction_errors_.shape == (2, 2) and list(s.lhalf_of_) == [-1] * 4 and fakes.instances[1].weight_calls == [0, 1, 2, 3]
    np.random.seed(99)
    assert_same(models[1], single(np.asarray(adata.X), 2, 1, w, None))


def test_validation(fakes, adata):
    for bad in ([], [-0.1], [0.5, float("nan")], [float("inf")]):
        with pytest.raises(ValueError):
            sal.models.KLNMFSweep([2], lhalf_weights=bad)
    with pytest.raises(ValueError):
        sal.models.KLNMFSweep([2], seeds=[0, 1], lhalf_weights=[0.5], stability=True)
    n_obs = adata.X.shape[0]
    with pytest.raises(ValueError):
        sal.models.KLNMFSweep([2], weights_kl=np.ones(n_obs + 1), **SETTINGS).fit(adata)
    with pytest.raises(ValueError):
        sal.models.KLNMFSweep([2], weights_kl=-np.ones(n_obs), **SETTINGS).fit(adata)
    with pytest.raises(TypeError):
        sal.models.KLNMFSweep([2], weights_kl="heavy", **SETTINGS).fit(adata)
    assert fakes.instances == []  # (refused before any batch exists)
    with pytest.raises(ValueError, match="constructor"):
        sal.models.KLNMFSweep([2], **SETTINGS).fit(adata, fitting_kwargs={"weights_lhalf": 0.5})
    with pytest.raises(ValueError):
        sal.models.KLNMFSweep([2], n_splits=2).suggest_penalty_heldout()
    assert sal.models.KLNMFSweep([2], n_splits=2, lhalf_weights=[0.1]).suggest_penalty_heldout() is None


def test_summaries_on_hand_made_arrays():
    s = sal.models.KLNMFSweep([2, 3, 4], seeds=[0, 1], lhalf_weights=[0.0, 1.0], n_splits=2)
    # (K, L, seeds, F): the seed of smaller training error per (K, penalty, f), the first on ties
    train = np.zeros((3, 2, 2, 2))
    train[:, :, 1, 0] = -1.0          # split 0: seed 1 wins; split 1: a tie, seed 0
    held = np.zeros((3, 2, 2, 2))
    held[:, :, 1, 0] = [[10, 9], [6, 6.5], [5, 8]]
    held[:, :, 0, 1] = [[12, 11], [8, 7.5], [5, 8]]
    held[:, :, 0, 0] = held[:, :, 1, 1] = 1e9  # (never taken)
    s._summarise_heldout(train, held)
    assert np.array_equal(s.heldout_mean_, [[11, 10], [7, 7], [5, 8]])
    assert np.allclose(s.heldout_sem_, [[1, 1], [1, 0.5], [0, 0]])
    s._fitted = True
    assert s.suggest_penalty_heldout() == (4, 0.0) and s.suggest_n_signatures_heldout() == 4
    assert s.suggest_penalty_heldout(one_standard_error=True) == (4, 0.0)  # (the minimum's standard error is 0)
    s.heldout_sem_[2, 0] = 2.0  # bound 7: the cells (3, 0.0), (3, 1.0), (4, 0.0) -- smallest K, then the largest penalty
    assert s.suggest_penalty_heldout(one_standard_error=True) == (3, 1.0)
    assert s.suggest_n_signatures_heldout(one_standard_error=True) == 3
    # today's three-axis arrays still summarise as before
    t = sal.models.KLNMFSweep([2, 3], seeds=[0, 1], n_splits=2)
    t._summarise_heldout(train[:2, 0], held[:2, 0])
    assert np.array_equal(t.heldout_mean_, [11, 7]) and np.allclose(t.heldout_sem_, [1, 1])
