"""KLNMFSweep with count splits on the MI355X: every member bit for bit the single fit on its own train split, and its
held-out divergences bit for bit what an engine on the test half computes.

Member (K, s, f) is compared with ``KLNMF(K, ..., objective_in_step=False).fit(AnnData(train_splits_[f]), None,
{"seed": s})`` by ``np.array_equal`` / list equality, in the style of tests/test_gpu_sweep_bootstrap.py.  The held-out
divergences come from the forward pass's per-sample mode, unchanged, reading another dataset and a scaled H
(``csrc/salnmf_batch.hip``): they equal ``Engine.samplewise_kl`` on ``max(test, EPSILON)``, W and ``max(c H, EPSILON)``.

Against the float64 host formula the tolerance is not tuned on the device: it is the spread, on the CPU, of the formula in
two feature orders about a longdouble evaluation, relative to the row's ``sum |x log(x / wh)| + x + wh``.  On these inputs
with oracle fits (``oracle/klnmf_oracle.py`` behind the fakes, host run) the largest spread is 4.59e-17 at N = 24, V = 96,
K = 1, 2, 5, 9 and 5.97e-17 at N = 70, V = 7, K = 3, recorded as ``HELD_SPREAD``; the device may lie 16 of them away, the
project's custom (DESIGN.md sections 13 and 14).  Each test prints the spread of its own run beside the device's distance."""
import numpy as np
import pytest

import _split_ref as ref
import salamander_amd as sal
from _fake_engine import FakeEngine
from _fake_split_batch_engine import FakeSplitBatchEngine
from oracle import klnmf_oracle as orc
from salamander_amd.models import signature_nmf, sweep

pytestmark = pytest.mark.gpu

EPSILON = 1.1920928955078125e-07
SETTINGS = dict(init_method="random", min_iterations=20, max_iterations=40, conv_test_freq=10)
SEEDS, F, P, SPLIT_SEED = [0, 1], 2, 0.5, 2024
HELD_SPREAD = {(24, 96): 4.6e-17, (70, 7): 6.0e-17}  # measured 4.59e-17 and 5.97e-17: see the module docstring


def planted(N, V, seed, depth=2000.0):
    """Poisson counts from 3 planted Dirichlet signatures."""
    rng = np.random.default_rng(seed)
    W = rng.dirichlet(np.full(V, 0.2), size=3)
    H = rng.dirichlet(np.full(3, 0.5), size=N) * depth
    return rng.poisson(H @ W).astype(float)


def single(X, K, seed, settings=SETTINGS):
    m = sal.models.KLNMF(K, objective_in_step=False, **settings)
    m.fit(sal.AnnData(np.array(X, copy=True)), None, {"seed": seed})
    m.compute_reconstruction_errors()
    m._engine.close()
    return m


def engine_heldout(model, test, p):
    """The fallback scorer of the sweep, spelled out: one engine on the clipped test half, W, and the scaled, clipped H."""
    c = (1.0 - p) / p
    X = np.maximum(test, EPSILON)
    H = np.maximum(c * np.asarray(model.adata.obsm["exposures"]), EPSILON)
    e = sal.Engine(X.shape[0], X.shape[1], model.n_signatures)
    try:
        e.upload_X(X), e.upload_W(np.asarray(model.asignatures.X)), e.upload_H(H)
        return np.asarray(e.samplewise_kl())
    finally:
        e.close()


def host_heldout(model, test, p, dtype=np.float64, perm=None):
    """``samplewise_kl_divergence(max(test, EPS), W, max(c H, EPS))`` in ``dtype`` with the features in the order ``perm``,
    and the row's scale ``sum |x log(x / wh)| + x + wh``."""
    c = (1.0 - p) / p
    perm = np.arange(test.shape[1]) if perm is None else perm
    X = np.maximum(test, EPSILON)[:, perm].astype(dtype)
    H = np.maximum(c * np.asarray(model.adata.obsm["exposures"]), EPSILON).astype(dtype)
    WH = H @ np.asarray(model.asignatures.X)[:, perm].astype(dtype)
    terms = X * np.log(X / WH)
    return (terms - X + WH).sum(axis=1), (np.abs(terms) + X + WH).sum(axis=1)


def spread_of(models, s, p):
    """Largest relative distance of the float64 formula, in two feature orders, from the longdouble evaluation."""
    worst = 0.0
    for m, f in zip(models, s.split_of_):
        test = s.test_splits_[f]
        ld, scale = host_heldout(m, test, p, np.longdouble)
        for perm in (None, np.random.default_rng(7).permutation(test.shape[1])):
            worst = max(worst, float(np.max(np.abs(host_heldout(m, test, p, perm=perm)[0] - ld) / scale)))
    return worst


def check_sweep(X, Ks, settings=SETTINGS):
    """(a), (b), (c) on one sweep."""
    s = sal.models.KLNMFSweep(Ks, seeds=SEEDS, n_splits=F, train_fraction=P, split_seed=SPLIT_SEED, **settings)
    models = s.fit(sal.AnnData(X.copy()))
    want_train, want_test = ref.split_counts(X, F, P, SPLIT_SEED)
    assert np.array_equal(s.train_splits_, want_train) and np.array_equal(s.test_splits_, want_test)
    members = [(K, sd, f) for K in Ks for sd in SEEDS for f in range(F)]
    assert len(models) == len(members) and list(s.split_of_) == [f for _, _, f in members] and s.batched_.all()
    worst = 0.0
    for got, (K, sd, f) in zip(models, members):
        want = single(s.train_splits_[f], K, sd, settings)
        # (a) the fit
        assert got.n_iterations_ == want.n_iterations_ and got.history["objective_function"] == want.history["objective_function"], (K, sd, f)
        assert np.array_equal(got.asignatures.X, want.asignatures.X) and np.array_equal(got.adata.obsm["exposures"], want.adata.obsm["exposures"]), (K, sd, f)
        assert np.array_equal(np.asarray(got.adata.obs["reconstruction_error"]), np.asarray(want.adata.obs["reconstruction_error"]))
        assert got.reconstruction_error == want.reconstruction_error
        assert np.array_equal(got.adata.X, np.maximum(s.train_splits_[f], EPSILON))
        # (b) the held-out divergences against the engine on the test half
        held = np.asarray(got.adata.obs["heldout_error"])
        assert np.array_equal(held, engine_heldout(want, s.test_splits_[f], P)), (K, sd, f)
        # (c) and against the float64 formula
        value, scale = host_heldout(want, s.test_splits_[f], P)
        worst = max(worst, float(np.max(np.abs(held - value) / scale)))
    spread = spread_of(models, s, P)
    tol = 16 * HELD_SPREAD[X.shape]
    print(f"N={X.shape[0]} V={X.shape[1]} Ks={list(Ks)}: host spread {spread:.3g}, device {worst:.3g}, tolerance {tol:.3g}")
    assert worst <= tol
    assert s.reconstruction_errors_.shape == s.heldout_errors_.shape == (len(Ks), len(SEEDS), F)
    assert np.array_equal(s.heldout_errors_.reshape(-1), [float(np.sum(np.asarray(m.adata.obs["heldout_error"]))) for m in models])
    assert {"split_s", "heldout_s"} <= set(s.timings_)
    return s


def test_members_and_heldout_errors_with_three_kernel_widths_in_one_launch():
    """(a), (b), (c): N = 24, V = 96, K = 1, 2, 5, 9 -- KS = 1, 2 and 4 share the held-out launch."""
    s = check_sweep(planted(24, 96, 1), [1, 2, 5, 9])
    assert s.suggest_n_signatures_heldout() in (1, 2, 5, 9) and np.isfinite(s.heldout_sem_).all()


def test_two_sample_groups_and_narrow_features():
    """(d): N = 70, V = 7 -- the NG = 2 workgroup of the step, pad columns in every slot."""
    check_sweep(planted(70, 7, 2), [3])


def test_a_fallback_member_in_the_same_sweep():
    """(e): K = 17 is outside the batch: fitted by KLNMF.fit on its train split, scored by a single engine."""
    X = planted(24, 96, 1)
    s = sal.models.KLNMFSweep([2, 17], seeds=SEEDS, n_splits=F, train_fraction=P, split_seed=SPLIT_SEED, **SETTINGS)
    models = s.fit(sal.AnnData(X.copy()))
    assert list(s.batched_) == [True] * 4 + [False] * 4
    for got, (K, sd, f) in zip(models, [(K, sd, f) for K in (2, 17) for sd in SEEDS for f in range(F)]):
        want = single(s.train_splits_[f], K, sd)
        assert np.array_equal(got.asignatures.X, want.asignatures.X) and np.array_equal(got.adata.obsm["exposures"], want.adata.obsm["exposures"])
        held = np.asarray(got.adata.obs["heldout_error"])
        assert np.isfinite(held).all() and np.array_equal(held, engine_heldout(want, s.test_splits_[f], P)), (K, sd, f)
    assert np.isfinite(s.heldout_errors_).all() and np.isfinite(s.heldout_mean_).all()


def test_without_splits_a_sweep_is_what_it_was():
    """(f)"""
    X = planted(24, 96, 1)
    a = sal.models.KLNMFSweep([2, 5], seeds=SEEDS, n_splits=0, train_fraction=0.8, split_seed=3, **SETTINGS)
    b = sal.models.KLNMFSweep([2, 5], seeds=SEEDS, **SETTINGS)
    ma, mb = a.fit(sal.AnnData(X.copy())), b.fit(sal.AnnData(X.copy()))
    for x, y in zip(ma, mb):
        assert np.array_equal(x.asignatures.X, y.asignatures.X) and np.array_equal(x.adata.obsm["exposures"], y.adata.obsm["exposures"])
        assert x.n_iterations_ == y.n_iterations_ and x.history["objective_function"] == y.history["objective_function"]
        assert np.array_equal(np.asarray(x.adata.obs["reconstruction_error"]), np.asarray(y.adata.obs["reconstruction_error"]))
        assert "heldout_error" not in x.adata.obs
    assert np.array_equal(a.reconstruction_errors_, b.reconstruction_errors_) and a.reconstruction_errors_.shape == (2, 2)
    assert set(a.timings_) == set(b.timings_) == {"total_s", "init_s", "batched_s", "fallback_s", "resample_s"}
    assert a.train_splits_ is None and list(a.split_of_) == [-1] * 4


def test_stability_counts_seeds_times_splits():
    """(g)"""
    X = planted(24, 96, 1)
    s = sal.models.KLNMFSweep([2, 3, 17], seeds=SEEDS, n_splits=F, stability=True, **SETTINGS)
    s.fit(sal.AnnData(X.copy()))
    assert np.isfinite(s.stability_mean_[:2]).all() and np.isnan(s.stability_mean_[2])
    assert s.assignments_[0].shape == (len(SEEDS) * F, 2) and np.isfinite(s.heldout_mean_).all()


def test_heldout_likelihood_selects_the_planted_number_of_signatures(monkeypatch):
    """(h): 3 planted signatures, N = 60, V = 96, K = 1 .. 6, F = 4, fits of exactly 200 steps.  The fixture was chosen on
    the CPU: the oracle (``oracle/klnmf_oracle.py`` behind the fakes, on the replica's splits) has its smallest
    ``heldout_mean_`` at K = 3, every other K at least 1 % above it (2 988.8 against 3 069.0 at K = 4, 2.7 %; asserted below).  The
    device must agree with the oracle's six numbers to rel 1e-4, the project's parity gate, and pick K = 3."""
    X = planted(60, 96, 0)
    kw = dict(seeds=SEEDS, init_method="random", n_splits=4, train_fraction=0.5, split_seed=0, min_iterations=200, max_iterations=200,
              conv_test_freq=200)
    s = sal.models.KLNMFSweep(range(1, 7), **kw)
    s.fit(sal.AnnData(X.copy()))
    assert s.batched_.all()
    monkeypatch.setattr(signature_nmf, "Engine", FakeEngine)
    monkeypatch.setattr(sweep, "Engine", FakeEngine)
    monkeypatch.setattr(sweep, "BatchEngine", FakeSplitBatchEngine)
    o = sal.models.KLNMFSweep(range(1, 7), **kw)
    o.fit(sal.AnnData(X.copy()))
    want = o.heldout_mean_
    print("oracle", want, "device", s.heldout_mean_, "rel", np.abs(s.heldout_mean_ - want) / want)
    assert np.delete(want, 2).min() >= 1.01 * want[2]
    assert np.array_equal(s.train_splits_, o.train_splits_) and np.array_equal(s.test_splits_, o.test_splits_)
    assert np.allclose(s.heldout_mean_, want, rtol=1e-4, atol=0.0)
    assert np.allclose(s.heldout_sem_, o.heldout_sem_, rtol=1e-3, atol=0.0)
    assert s.suggest_n_signatures_heldout() == 3 and o.suggest_n_signatures_heldout() == 3
