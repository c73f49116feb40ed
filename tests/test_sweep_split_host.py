"""KLNMFSweep with count splits on the CPU: member order, the held-out results and the selection rules, on oracle-backed
fakes (``_fake_split_batch_engine``).

Every member is compared with its single fit on the MI355X in tests/test_gpu_sweep_split.py."""

import os

import numpy as np
import pytest

import _split_ref as ref
import salamander_amd as sal
from _fake_engine import FakeEngine
from _fake_split_batch_engine import FakeSplitBatchEngine
from conftest import REF_FIX, read_counts
from oracle import klnmf_oracle as orc
from salamander_amd.models import signature_nmf, sweep

EPSILON = 1.1920928955078125e-07
SETTINGS = dict(init_method="random", min_iterations=20, max_iterations=40, conv_test_freq=10, tol=1e-4)
TODAYS_KEYS = {"total_s", "init_s", "batched_s", "fallback_s", "resample_s"}


@pytest.fixture
def fakes(monkeypatch):
    monkeypatch.setattr(signature_nmf, "Engine", FakeEngine)
    monkeypatch.setattr(sweep, "Engine", FakeEngine)
    monkeypatch.setattr(sweep, "BatchEngine", FakeSplitBatchEngine)
    monkeypatch.setattr(sweep, "split_counts", lambda X, F, p, seed, device=0: ref.split_counts(X, F, p, seed))
    FakeSplitBatchEngine.instances = []
    FakeSplitBatchEngine.planted = None
    yield FakeSplitBatchEngine
    FakeSplitBatchEngine.planted = None


@pytest.fixture
def adata():
    return sal.AnnData(read_counts(os.path.join(REF_FIX, "klnmf", "counts.csv")).T)


def single(X, K, init_kwargs=None):
    m = sal.models.KLNMF(K, objective_in_step=False, **SETTINGS)
    m.fit(sal.AnnData(X.copy()), None, init_kwargs)
    m.compute_reconstruction_errors()
    return m


def heldout(model, test, p):
    c = (1.0 - p) / p
    H = np.maximum(c * model.adata.obsm["exposures"], EPSILON)
    return orc.samplewise_kl_divergence(np.maximum(test, EPSILON).T, model.asignatures.X.T, H.T)


def test_member_order_own_split_and_heldout_results(fakes, adata):
    X_before = np.array(adata.X, copy=True)
    Ks, seeds, F, p = [1, 3, 2], [0, 1], 2, 0.8
    s = sal.models.KLNMFSweep(Ks, seeds=seeds, n_splits=F, train_fraction=p, split_seed=5, **SETTINGS)
    assert s.suggest_n_signatures_heldout() is None  # (before fit)
    models = s.fit(adata)
    assert np.array_equal(adata.X, X_before) and "heldout_error" not in adata.obs  # the caller's data is untouched
    (engine,) = fakes.instances
    assert engine.split_calls == [(F, p, 5)] and engine.resample_calls == [] and engine.closed
    # K-major, seed-middle, split-minor
    assert [m.n_signatures for m in models] == [K for K in Ks for _ in range(len(seeds) * F)]
    assert list(s.split_of_) == list(range(F)) * (len(Ks) * len(seeds)) and engine.dataset == list(s.split_of_)
    assert list(s.resample_of_) == [-1] * len(models) and s.resamples_ is None
    want_train, want_test = ref.split_counts(X_before, F, p, 5)
    assert np.array_equal(s.train_splits_, want_train) and np.array_equal(s.test_splits_, want_test)
    # one held-out call over all batched members, each against the test half of its own split
    assert engine.heldout_calls == [(list(range(len(models))), [F + f for f in s.split_of_], p)]
    assert s.batched_.all()
    assert s.reconstruction_errors_.shape == s.heldout_errors_.shape == (len(Ks), len(seeds), F)
    assert s.heldout_mean_.shape == s.heldout_sem_.shape == (len(Ks),) and np.isfinite(s.heldout_mean_).all() and np.isfinite(s.heldout_sem_).all()
    assert set(s.timings_) == TODAYS_KEYS | {"split_s", "heldout_s"}
    np.random.seed(99)
    members = [(K, sd, f) for K in Ks for sd in seeds for f in range(F)]
    for got, (K, sd, f), total in zip(models, members, s.heldout_errors_.reshape(-1)):
        want = single(s.train_splits_[f], K, {"seed": sd})
        assert np.array_equal(got.asignatures.X, want.asignatures.X) and np.array_equal(got.adata.obsm["exposures"], want.adata.obsm["exposures"])
        assert got.n_iterations_ == want.n_iterations_ and got.history["objective_function"] == want.history["objective_function"]
        assert np.array_equal(got.adata.X, s.train_splits_[f].clip(EPSILON))
        held = np.asarray(got.adata.obs["heldout_error"])
        assert np.array_equal(held, heldout(want, s.test_splits_[f], p)) and total == held.sum()
    # the summary follows the rule, from the sweep's own numbers
    best = s.reconstruction_errors_.argmin(axis=1)
    chosen = np.array([[s.heldout_errors_[k, best[k, f], f] for f in range(F)] for k in range(len(Ks))])
    assert np.array_equal(s.heldout_mean_, chosen.mean(axis=1))
    assert np.array_equal(s.heldout_sem_, chosen.std(axis=1, ddof=1) / np.sqrt(F))
    assert s.suggest_n_signatures_heldout() == Ks[int(np.argmin(s.heldout_mean_))]


def plant(Ks, n_seeds, F, train, held):
    FakeSplitBatchEngine.planted = {"train": np.asarray(train, dtype=float).reshape(-1), "heldout": np.asarray(held, dtype=float).reshape(-1)}
    assert len(FakeSplitBatchEngine.planted["train"]) == len(Ks) * n_seeds * F


def test_the_seed_is_selected_on_training_error_with_ties_to_the_lowest_index(fakes, adata):
    """Planted (K, seed, f) numbers: 3 values of K, 3 seeds, F = 2."""
    Ks, seeds, F = [2, 3, 4], [7, 8, 9], 2
    train = [[[5.0, 3.0], [4.0, 3.0], [4.0, 9.0]],   # K = 2: f = 0 -> seeds 1, 2 tie: seed 1; f = 1 -> seeds 0, 1 tie: seed 0
             [[1.0, 2.0], [0.5, 2.5], [0.7, 1.0]],   # K = 3: f = 0 -> seed 1; f = 1 -> seed 2
             [[6.0, 6.0], [6.0, 6.0], [6.0, 6.0]]]   # K = 4: all tie -> seed 0 twice
    held = [[[1.0, 20.0], [10.0, 2.0], [3.0, 4.0]],
            [[9.0, 9.0], [8.0, 9.0], [9.0, 6.0]],
            [[7.5, 8.5], [1.0, 1.0], [1.0, 1.0]]]
    plant(Ks, 3, F, train, held)
    s = sal.models.KLNMFSweep(Ks, seeds=seeds, n_splits=F, **SETTINGS)
    s.fit(adata)
    assert np.array_equal(s.reconstruction_errors_, train) and np.array_equal(s.heldout_errors_, held)
    assert np.array_equal(s.heldout_mean_, [15.0, 7.0, 8.0])  # (10 + 20) / 2, (8 + 6) / 2, (7.5 + 8.5) / 2
    assert np.allclose(s.heldout_sem_, [np.std([10.0, 20.0], ddof=1) / np.sqrt(2), np.std([8.0, 6.0], ddof=1) / np.sqrt(2), 0.5], rtol=1e-15)
    assert s.suggest_n_signatures_heldout() == 3
    # one standard error of the minimum: 7 + 1 = 8 admits K = 4 (mean 8) but not K = 2 (15): the smallest admitted K is 3
    assert s.suggest_n_signatures_heldout(one_standard_error=True) == 3


def test_the_one_standard_error_rule_prefers_the_smaller_model(fakes, adata):
    Ks, F = [1, 2, 3, 4], 3
    train = np.ones((4, 1, F))
    held = [[[30.0, 31.0, 32.0]], [[10.5, 11.0, 12.1]], [[9.0, 11.0, 10.0]], [[10.0, 10.0, 10.3]]]
    plant(Ks, 1, F, train, held)
    s = sal.models.KLNMFSweep(Ks, n_splits=F, **SETTINGS)
    s.fit(adata)
    assert s.heldout_errors_.shape == (4, 1, F)
    assert np.allclose(s.heldout_mean_, [31.0, 11.2, 10.0, 10.1]) and np.isclose(s.heldout_sem_[2], 1.0 / np.sqrt(3.0))
    assert s.suggest_n_signatures_heldout() == 3
    # 10 + 0.577 admits K = 4 (10.1) and not K = 2 (11.2): still 3; with a wider minimum K = 2 comes in
    assert s.suggest_n_signatures_heldout(one_standard_error=True) == 3
    held[2] = [[7.0, 13.0, 10.0]]  # the same mean, standard error sqrt(3)
    plant(Ks, 1, F, train, held)
    s.fit(adata)
    assert s.suggest_n_signatures_heldout() == 3 and s.suggest_n_signatures_heldout(one_standard_error=True) == 2


def test_one_split_has_no_standard_error(fakes, adata):
    plant([2, 3], 2, 1, [[[2.0], [1.0]], [[1.0], [1.0]]], [[[5.0], [6.0]], [[4.0], [9.0]]])
    s = sal.models.KLNMFSweep([2, 3], seeds=[0, 1], n_splits=1, **SETTINGS)
    s.fit(adata)
    assert s.heldout_errors_.shape == (2, 2, 1) and np.array_equal(s.heldout_mean_, [6.0, 4.0]) and np.isnan(s.heldout_sem_).all()
    assert s.suggest_n_signatures_heldout() == 3 and s.suggest_n_signatures_heldout(one_standard_error=True) == 3


def test_a_fallback_member_is_scored_by_a_single_engine(fakes, adata):
    """17 signatures are outside the batched kernel: that member runs KLNMF.fit on its train split and is scored by an
    engine on the test half; with no member in reach there is no batch and the splits come from the stand-alone entry."""
    s = sal.models.KLNMFSweep([2, 17], seeds=[4], n_splits=2, **SETTINGS)
    models = s.fit(adata)
    assert list(s.batched_) == [True, True, False, False] and list(s.split_of_) == [0, 1, 0, 1]
    (engine,) = fakes.instances
    assert engine.heldout_calls == [([0, 1], [2, 3], 0.5)]
    for got, K, f in zip(models, [2, 2, 17, 17], s.split_of_):
        want = single(s.train_splits_[f], K, {"seed": 4})
        assert np.array_equal(got.asignatures.X, want.asignatures.X)
        assert np.array_equal(np.asarray(got.adata.obs["heldout_error"]), heldout(want, s.test_splits_[f], 0.5))
    fakes.instances = []
    s = sal.models.KLNMFSweep([17], seeds=[4], n_splits=2, split_seed=3, **SETTINGS)
    models = s.fit(adata)
    assert not fakes.instances and not s.batched_.any() and s.heldout_errors_.shape == (1, 1, 2)
    want_train, want_test = ref.split_counts(np.asarray(adata.X), 2, 0.5, 3)
    assert np.array_equal(s.train_splits_, want_train) and np.array_equal(s.test_splits_, want_test)
    assert np.isfinite(s.heldout_errors_).all() and set(s.timings_) == TODAYS_KEYS | {"split_s", "heldout_s"}


def test_without_splits_nothing_changes(fakes, adata):
    s = sal.models.KLNMFSweep([1, 2], seeds=[0, 1], n_splits=0, **SETTINGS)
    with pytest.raises(ValueError, match="n_splits"):
        s.suggest_n_signatures_heldout()
    models = s.fit(adata)
    (engine,) = fakes.instances
    assert engine.split_calls == [] and engine.heldout_calls == [] and s.train_splits_ is None and s.test_splits_ is None
    assert list(s.split_of_) == [-1] * 4 and list(s.resample_of_) == [-1] * 4
    assert s.reconstruction_errors_.shape == (2, 2) and set(s.timings_) == TODAYS_KEYS
    assert all("heldout_error" not in m.adata.obs for m in models)
    with pytest.raises(ValueError, match="n_splits"):
        s.suggest_n_signatures_heldout()
    with pytest.raises(ValueError, match="exclude each other"):
        sal.models.KLNMFSweep([2], n_splits=1, n_resamples=1)


def test_bad_counts_are_refused_before_the_device(fakes, adata):
    X = np.array(adata.X, dtype=float)
    X[5, 7] += 0.5
    with pytest.raises(ValueError, match="row 5"):
        sal.models.KLNMFSweep([2], n_splits=2, **SETTINGS).fit(sal.AnnData(X))
    assert fakes.instances == []
