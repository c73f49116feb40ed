"""Signature stability on the CPU: the NumPy replica of the device's contract (tests/_stability_ref.py) against
scikit-learn's silhouettes, the reference's pair matching and planted structure, and KLNMFSweep's stability logic on
oracle-backed fakes.  The device is compared with the replica in tests/test_gpu_stability.py."""

import os

import numpy as np
import pytest

import _resample_ref
import _stability_ref as ref
import salamander_amd as sal
from _fake_engine import FakeEngine
from _fake_stability_batch_engine import FakeStabilityBatchEngine
from conftest import GOLDEN, REF_FIX, read_counts
from salamander_amd.models import signature_nmf, sweep
from salamander_amd.stability import StabilityResult


# ------------------------------------------------------------------ the replica
@pytest.mark.parametrize("K,M,cv", [(2, 7, 0.3), (5, 24, 0.3), (16, 30, 0.6)])
def test_silhouettes_equal_sklearn(K, M, cv):
    from sklearn.metrics import silhouette_samples

    sigs, _ = ref.planted(K, M, 96, cv, seed=K)
    r = ref.stability(sigs)
    want = silhouette_samples(r.points.reshape(M * K, -1), np.tile(np.arange(K), M), metric="cosine").reshape(M, K)
    print(f"K={K} M={M}: max |silhouette - sklearn| = {np.abs(r.silhouette - want).max():.3g}")
    assert np.abs(r.silhouette - want).max() <= 1e-12


def test_first_round_of_a_pair_equals_the_reference_matching():
    """stability_pairs.npz: what the reference's match_signatures_pair returned (tests/golden/make_stability_golden.py)."""
    d = np.load(os.path.join(GOLDEN, "stability_pairs.npz"))
    assert int(d["n_pairs"]) >= 8
    for i in range(int(d["n_pairs"])):
        first, second, indices = d[f"first_{i}"], d[f"second_{i}"], d[f"indices_{i}"]
        r = ref.stability(np.stack([first, second]), max_rounds=1)  # anchor: member 0, i.e. `first`
        assert r.margins.min() > 1e-6
        assert np.array_equal(r.assignments[0], np.arange(len(first)))
        assert np.array_equal(r.assignments[1], indices), i


@pytest.mark.parametrize("cv", [0.05, 0.3])
@pytest.mark.parametrize("K,M", [(5, 24), (8, 64), (16, 100)])
def test_planted_permutations_come_back_in_two_rounds(K, M, cv):
    sigs, perms = ref.planted(K, M, 96, cv, seed=K + M)
    r = ref.stability(sigs)
    assert r.margins.min() > 1e-6
    print(f"K={K} M={M} cv={cv}: margin {r.margins.min():.3g}, smallest a {r.a.min():.3g}, minimum cluster stability {r.stability_min:.4f}")
    assert np.array_equal(r.assignments, ref.expected_assignments(perms, 0))
    assert r.n_rounds == 2 and r.converged
    assert r.stability_min > (0.99 if cv == 0.05 else 0.8)
    assert np.allclose(r.consensus.sum(axis=1), 1.0)


def test_replica_round_cap_and_single_signature():
    sigs, _ = ref.planted(8, 24, 96, 1.0, 4, mix=0.5)
    full, one = ref.stability(sigs), ref.stability(sigs, max_rounds=1)
    assert full.n_rounds > 2 and full.converged and one.n_rounds == 1 and not one.converged
    assert not np.array_equal(full.assignments, one.assignments)
    r = ref.stability(ref.planted(1, 5, 96, 0.3, 0)[0])
    assert np.isnan(r.b).all() and np.array_equal(r.silhouette, np.ones((5, 1))) and r.stability_mean == 1.0 and r.n_rounds == 2


# ------------------------------------------------------------------ validation that needs no device
def test_signature_stability_refuses_bad_input_before_the_device():
    good, _ = ref.planted(4, 5, 96, 0.3, seed=1)
    zero, nan = good.copy(), good.copy()
    zero[2, 1] = 0.0
    nan[3, 0, 7] = np.inf
    for bad in (np.ones((3, 17, 96)), np.ones((3, 4, 97)), good[:1], zero, nan, [good, good[:, :, :83]], good[0], []):
        with pytest.raises(ValueError):
            sal.signature_stability(bad)
    for kwargs in ({"max_rounds": 0}, {"max_rounds": 2.5}, {"errors": [1.0, 2.0]}, {"errors": [1.0, 2.0, np.nan, 1.0, 1.0]}):
        with pytest.raises(ValueError):
            sal.signature_stability(good, **kwargs)


# ------------------------------------------------------------------ the sweep's host logic on fakes
@pytest.fixture
def fakes(monkeypatch):
    monkeypatch.setattr(signature_nmf, "Engine", FakeEngine)
    monkeypatch.setattr(sweep, "BatchEngine", FakeStabilityBatchEngine)
    monkeypatch.setattr(sweep, "resample_counts", lambda X, R, seed, device=0: _resample_ref.resample_counts(X, R, seed))
    FakeStabilityBatchEngine.instances = []
    return FakeStabilityBatchEngine


@pytest.fixture
def adata():
    return sal.AnnData(read_counts(os.path.join(REF_FIX, "klnmf", "counts.csv")).T)


SETTINGS = dict(init_method="random", min_iterations=30, max_iterations=40, conv_test_freq=10, tol=1e-4)


def test_construction_needs_two_members_per_k():
    for kwargs in ({}, {"seeds": [3]}, {"n_resamples": 1}, {"seeds": [3], "n_resamples": 1}):
        with pytest.raises(ValueError, match="two members"):
            sal.models.KLNMFSweep([2, 3], stability=True, **kwargs)
        sal.models.KLNMFSweep([2, 3], **kwargs)  # (fine without stability)
    for kwargs in ({"seeds": [0, 1]}, {"n_resamples": 2}, {"seeds": [0, 1], "n_resamples": 3}):
        sal.models.KLNMFSweep([2, 3], stability=True, **kwargs)
    with pytest.raises(ValueError):
        sal.models.KLNMFSweep([2], seeds=[0, 1], stability=True, stability_max_rounds=0)
    with pytest.raises(ValueError, match="stability=True"):
        sal.models.KLNMFSweep([2], seeds=[0, 1]).suggest_n_signatures()


def test_groups_member_order_and_errors(fakes, adata):
    s = sal.models.KLNMFSweep([2, 3, 4], seeds=[5, 6], n_resamples=3, stability=True, stability_max_rounds=7, **SETTINGS)
    models = s.fit(adata)
    b = fakes.instances[-1]
    assert b.closed and len(b.stability_calls) == 1
    groups, errors, max_rounds = b.stability_calls[0]
    assert groups == [list(range(0, 6)), list(range(6, 12)), list(range(12, 18))] and max_rounds == 7  # K-major, sweep order
    assert errors == [[m.reconstruction_error for m in models[6 * g : 6 * g + 6]] for g in range(3)]
    assert np.array_equal(np.array(errors), s.reconstruction_errors_.reshape(3, 6))
    assert s.stability_mean_.shape == s.stability_min_.shape == (3,) and "stability_s" in s.timings_
    for g, K in enumerate([2, 3, 4]):
        want = ref.stability(np.stack([m.asignatures.X for m in models[6 * g : 6 * g + 6]]), errors[g], 7, margins=False)
        assert np.array_equal(s.assignments_[g], want.assignments) and s.assignments_[g].shape == (6, K)
        assert np.array_equal(s.silhouettes_[g], want.silhouette) and np.array_equal(s.consensus_signatures_[g], want.consensus)
        assert np.array_equal(s.cluster_stability_[g], want.cluster_stability) and s.cluster_stability_[g].shape == (K,)
        assert s.stability_mean_[g] == want.stability_mean and s.stability_min_[g] == want.stability_min
        assert s.stability_rounds_[g] == want.n_rounds and s.stability_converged_[g] == want.converged
    assert s.suggest_n_signatures() == ref.suggest([2, 3, 4], s.stability_mean_, s.stability_min_)


def test_groups_out_of_the_kernels_reach_get_nan(fakes, adata, monkeypatch):
    calls = []

    def stand_alone(signatures, errors=None, max_rounds=20, device=0):
        calls.append(([np.shape(x) for x in signatures], errors, max_rounds))
        out = []
        for x, e in zip(signatures, errors):
            r = ref.stability(x, e, max_rounds, margins=False)
            out.append(StabilityResult(r.assignments, r.n_rounds, r.converged, r.consensus, r.a, r.b, r.silhouette, r.cluster_stability,
                                       r.stability_mean, r.stability_min))
        return out

    monkeypatch.setattr(sweep, "signature_stability", stand_alone)
    monkeypatch.setattr(sweep, "STABILITY_MAX_SIGNATURES", 2)  # (as if K = 3 were beyond the kernel)
    s = sal.models.KLNMFSweep([2, 3], seeds=[0, 1], stability=True, **SETTINGS)
    s.fit(adata)
    assert fakes.instances[-1].stability_calls[0][0] == [[0, 1]] and not calls  # only the group in reach, in place
    assert np.isfinite(s.stability_mean_[0]) and np.isnan(s.stability_mean_[1]) and np.isnan(s.stability_min_[1])
    assert s.consensus_signatures_[1] is None and s.assignments_[1] is None and s.silhouettes_[1] is None and s.cluster_stability_[1] is None
    assert s.stability_rounds_[1] == 0 and not s.stability_converged_[1]
    assert s.suggest_n_signatures(-1.0, -1.0) == 2  # a NaN passes no threshold
    # members outside the batch (here: as if no batch could be made): the stand-alone form on the models' signatures
    monkeypatch.setattr(sweep, "STABILITY_MAX_SIGNATURES", 16)
    monkeypatch.setattr(sweep, "MAX_SAMPLES", 4)
    s = sal.models.KLNMFSweep([2, 3], seeds=[0, 1], stability=True, stability_max_rounds=5, **SETTINGS)
    models = s.fit(adata)
    assert not s.batched_.any() and len(calls) == 1
    assert calls[0][0] == [(2, 2, 96), (2, 3, 96)] and calls[0][2] == 5
    assert calls[0][1] == [[m.reconstruction_error for m in models[:2]], [m.reconstruction_error for m in models[2:]]]
    assert np.isfinite(s.stability_mean_).all()


def test_suggest_n_signatures_on_hand_made_scores():
    s = sal.models.KLNMFSweep([2, 3, 4, 5, 6], seeds=[0, 1], stability=True)
    s.stability_mean_ = np.array([0.99, 0.95, 0.85, 0.79, np.nan])
    s.stability_min_ = np.array([0.90, 0.10, 0.25, 0.70, np.nan])
    assert s.suggest_n_signatures() == 4
    assert s.suggest_n_signatures(min_stability=0.3) == 2
    assert s.suggest_n_signatures(mean_stability=0.75) == 5
    assert s.suggest_n_signatures(mean_stability=0.9, min_stability=0.05) == 3
    assert s.suggest_n_signatures(mean_stability=0.995) is None
    s.ns_signatures = [6, 5, 4, 3, 2]  # the largest K, not the last entry
    s.stability_mean_, s.stability_min_ = s.stability_mean_[::-1], s.stability_min_[::-1]
    assert s.suggest_n_signatures() == 4


@pytest.mark.parametrize("seeds,R", [([0, 1], 0), (None, 2)])
def test_stability_leaves_every_other_output_alone(fakes, adata, seeds, R):
    plain = sal.models.KLNMFSweep([1, 2, 4], seeds=seeds, n_resamples=R, **SETTINGS)
    np.random.seed(99)  # (the random method without a seed draws from the legacy RNG: both sweeps start it alike)
    a = plain.fit(adata)
    assert fakes.instances[-1].stability_calls == [] and "stability_s" not in plain.timings_
    assert set(plain.timings_) == {"total_s", "init_s", "batched_s", "fallback_s", "resample_s"}
    with_stability = sal.models.KLNMFSweep([1, 2, 4], seeds=seeds, n_resamples=R, stability=True, **SETTINGS)
    np.random.seed(99)
    b = with_stability.fit(adata)
    assert set(with_stability.timings_) == set(plain.timings_) | {"stability_s"}
    for x, y in zip(a, b):
        assert np.array_equal(x.asignatures.X, y.asignatures.X) and np.array_equal(x.adata.obsm["exposures"], y.adata.obsm["exposures"])
        assert x.history["objective_function"] == y.history["objective_function"] and x.n_iterations_ == y.n_iterations_
    assert np.array_equal(plain.reconstruction_errors_, with_stability.reconstruction_errors_)
    assert np.array_equal(plain.batched_, with_stability.batched_) and np.array_equal(plain.resample_of_, with_stability.resample_of_)
    assert plain.member_steps_ == with_stability.member_steps_
    assert (plain.resamples_ is None) == (with_stability.resamples_ is None)
    if R:
        assert np.array_equal(plain.resamples_, with_stability.resamples_)
