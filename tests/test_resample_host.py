"""Bootstrap resampling on the CPU: the NumPy replica of the device's resampler against the generator's published known
answers and the properties of the contract, and KLNMFSweep's resampling logic on oracle-backed fakes.

The device itself is compared with the replica entry by entry in tests/test_gpu_resample.py, and every bootstrap member
with its single fit in tests/test_gpu_sweep_bootstrap.py."""

import os

import numpy as np
import pytest

import _resample_ref as ref
import salamander_amd as sal
from _fake_engine import FakeEngine
from _fake_resample_batch_engine import FakeResampleBatchEngine
from conftest import GOLDEN, REF_FIX, read_counts
from salamander_amd.models import signature_nmf, sweep


# ------------------------------------------------------------------ the generator and the contract
@pytest.mark.parametrize("ctr,key,want", [
    ((0, 0, 0, 0), (0, 0), (0x6627E8D5, 0xE169C58D, 0xBC57AC4C, 0x9B00DBD8)),
    ((0xFFFFFFFF,) * 4, (0xFFFFFFFF,) * 2, (0x408F276D, 0x41C83B0E, 0xA20BC7C6, 0x6D5451FD)),
    ((0x243F6A88, 0x85A308D3, 0x13198A2E, 0x03707344), (0xA4093822, 0x299F31D0), (0xD16CFE09, 0x94FDCCEB, 0x5001E420, 0x24126EA1)),
])
def test_philox_known_answers(ctr, key, want):
    """Random123's kat_vectors for philox4x32-10."""
    got = ref.philox4x32_10(*[np.array([c]) for c in ctr], *key)
    assert tuple(int(g[0]) for g in got) == want


@pytest.fixture(scope="module")
def pcawg24():
    return read_counts(os.path.join(GOLDEN, "pcawg_breast_sbs.csv")).T.values[:24].astype(float)


def test_totals_zero_cells_and_independence_of_the_number_of_resamples(pcawg24):
    X = pcawg24.copy()
    X[3] = 0  # a sample without mutations stays empty
    Y = ref.resample_counts(X, 5, seed=11)
    assert Y.shape == (5, 24, 96) and np.array_equal(Y, np.floor(Y)) and (Y >= 0).all()
    assert np.array_equal(Y.sum(axis=2), np.broadcast_to(X.sum(axis=1), (5, 24)))
    assert (Y[:, X == 0] == 0).all()
    assert np.array_equal(ref.resample_counts(X, 2, seed=11), Y[:2])  # resample r does not depend on R
    assert not np.array_equal(Y[0], Y[1]) and not np.array_equal(ref.resample_counts(X, 1, seed=12)[0], Y[0])
    assert not np.array_equal(ref.resample_counts(X, 1, seed=11 + 2**32)[0], Y[0])  # the key's high word counts


@pytest.mark.parametrize("seed", [2024, 0, 7])
def test_resamples_follow_the_observed_spectra(pcawg24, seed):
    """Pearson's chi-square of the pooled resamples (R = 8) against R X over the non-zero cells, one multinomial per row:
    dof = cells - rows = 2279, z = (chi2 - dof) / sqrt(2 dof).  The replica gives z = 1.88, 1.82, 0.66 for seeds 2024, 0, 7;
    numpy's Generator.multinomial reached mean 0.03, sd 1.03, max 3.83 on the same statistic in 400 runs.  A biased bin
    search moves z by tens."""
    R = 8
    Y = ref.resample_counts(pcawg24, R, seed).sum(axis=0)
    cells = pcawg24 > 0
    E = R * pcawg24
    chi2 = float((((Y - E) ** 2)[cells] / E[cells]).sum())
    dof = int(cells.sum()) - len(pcawg24)
    z = (chi2 - dof) / np.sqrt(2 * dof)
    print(f"seed {seed}: chi2 {chi2:.1f}, dof {dof}, z {z:.3f}")
    assert dof == 2279
    assert abs(z) < 4.5, z


# ------------------------------------------------------------------ the sweep's host logic on fakes
@pytest.fixture
def fakes(monkeypatch):
    monkeypatch.setattr(signature_nmf, "Engine", FakeEngine)
    monkeypatch.setattr(sweep, "BatchEngine", FakeResampleBatchEngine)
    monkeypatch.setattr(sweep, "resample_counts", lambda X, R, seed, device=0: ref.resample_counts(X, R, seed))
    FakeResampleBatchEngine.instances = []
    return FakeResampleBatchEngine


@pytest.fixture
def adata():
    return sal.AnnData(read_counts(os.path.join(REF_FIX, "klnmf", "counts.csv")).T)


SETTINGS = dict(min_iterations=20, max_iterations=57, conv_test_freq=10, tol=1e-4)


def single(X, K, settings, init_kwargs=None):
    m = sal.models.KLNMF(K, objective_in_step=False, **settings)
    m.fit(sal.AnnData(X.copy()), None, init_kwargs)
    m.compute_reconstruction_errors()
    return m


def assert_same(a, b):
    assert a.n_signatures == b.n_signatures
    assert np.array_equal(a.asignatures.X, b.asignatures.X)
    assert np.array_equal(a.adata.obsm["exposures"], b.adata.obsm["exposures"])
    assert a.history["objective_function"] == b.history["objective_function"]
    assert a.n_iterations_ == b.n_iterations_
    assert np.array_equal(np.asarray(a.adata.obs["reconstruction_error"]), np.asarray(b.adata.obs["reconstruction_error"]))


@pytest.mark.parametrize("init_method,seeds", [("nndsvd", None), ("random", [0, 1])])
def test_member_order_shapes_and_own_resample(fakes, adata, init_method, seeds):
    settings = dict(SETTINGS, init_method=init_method)
    X_before = np.array(adata.X, copy=True)
    Ks, R, n_seeds = [1, 3, 2], 3, max(1, len(seeds or []))
    s = sal.models.KLNMFSweep(Ks, seeds=seeds, n_resamples=R, resample_seed=5, **settings)
    models = s.fit(adata)
    assert np.array_equal(adata.X, X_before) and "exposures" not in adata.obsm  # the caller's data is untouched
    (engine,) = fakes.instances
    assert engine.resample_calls == [(R, 5)] and engine.closed
    # K-major, seed-middle, resample-minor
    assert [m.n_signatures for m in models] == [K for K in Ks for _ in range(n_seeds * R)]
    assert list(s.resample_of_) == list(range(R)) * (len(Ks) * n_seeds) and engine.dataset == list(s.resample_of_)
    assert s.batched_.all() and s.reconstruction_errors_.shape == (len(Ks), n_seeds, R)
    assert np.array_equal(s.reconstruction_errors_.reshape(-1), [m.reconstruction_error for m in models])
    assert np.array_equal(s.resamples_, ref.resample_counts(X_before, R, 5)) and "resample_s" in s.timings_
    # every member was initialised on, and fits, its own resample: bit for bit the single fit of that matrix
    np.random.seed(99)
    want = [single(s.resamples_[r], K, settings, None if sd is None else {"seed": sd}) for K in Ks for sd in (seeds or [None]) for r in range(R)]
    for got, ref_model, r in zip(models, want, s.resample_of_):
        assert_same(got, ref_model)
        assert np.array_equal(got.adata.X, s.resamples_[r].clip(1.1920928955078125e-07))
        assert list(got.adata.obs_names) == list(adata.obs_names) and list(got.adata.var_names) == list(adata.var_names)
    assert len({m.reconstruction_error for m in models[:R]}) == R  # (the resamples are different problems)


def test_fallback_members_and_no_batch_at_all(fakes, adata):
    """17 signatures are outside the batched kernel: that member runs KLNMF.fit on its resample, in its place; when no
    member is in reach there is no batch and the resamples come from the stand-alone entry."""
    settings = dict(SETTINGS, init_method="random")
    s = sal.models.KLNMFSweep([2, 17], seeds=[4], n_resamples=2, **settings)
    models = s.fit(adata)
    assert list(s.batched_) == [True, True, False, False] and list(s.resample_of_) == [0, 1, 0, 1]
    for got, K, r in zip(models, [2, 2, 17, 17], s.resample_of_):
        assert_same(got, single(s.resamples_[r], K, settings, {"seed": 4}))
    fakes.instances = []
    s = sal.models.KLNMFSweep([17], seeds=[4], n_resamples=2, **settings)
    models = s.fit(adata)
    assert not fakes.instances and not s.batched_.any() and s.reconstruction_errors_.shape == (1, 1, 2)
    assert np.array_equal(s.resamples_, ref.resample_counts(np.asarray(adata.X), 2, 0))
    for got, r in zip(models, (0, 1)):
        assert_same(got, single(s.resamples_[r], 17, settings, {"seed": 4}))


def test_without_resamples_nothing_changes(fakes, adata):
    s = sal.models.KLNMFSweep([1, 2], seeds=[0, 1], init_method="random", n_resamples=0, **SETTINGS)
    models = s.fit(adata)
    (engine,) = fakes.instances
    assert engine.resample_calls == [] and s.resamples_ is None and list(s.resample_of_) == [-1] * 4
    assert s.reconstruction_errors_.shape == (2, 2) and s.timings_["resample_s"] == 0.0
    for got, (K, sd) in zip(models, [(1, 0), (1, 1), (2, 0), (2, 1)]):
        assert_same(got, single(np.asarray(adata.X), K, dict(SETTINGS, init_method="random"), {"seed": sd}))


def test_counts_are_validated_before_the_engine_exists(fakes, adata):
    for bad in (-1, 1.5, True, 70000):
        with pytest.raises(ValueError, match="n_resamples"):
            sal.models.KLNMFSweep([2], n_resamples=bad)
    for bad in (-1, 2**64, 0.5):
        with pytest.raises(ValueError, match="seed"):
            sal.models.KLNMFSweep([2], n_resamples=2, resample_seed=bad)
    s = sal.models.KLNMFSweep([2, 3], n_resamples=2, **SETTINGS)
    X = np.array(adata.X, dtype=float)
    cases = []
    Y = X.copy(); Y[5, 7] += 0.5; cases.append((Y, "row 5"))
    Y = X.copy(); Y[2, 0] = -1.0; Y[9, 1] = 0.25; cases.append((Y, "row 2"))
    Y = X.copy(); Y[4, :2] = 2.0**31; cases.append((Y, "row 4"))
    Y = X.copy(); Y[6, 3] = np.nan; cases.append((Y, "row 6"))
    for Y, row in cases:
        with pytest.raises(ValueError, match=row):
            s.fit(sal.AnnData(Y))
    assert fakes.instances == []  # nothing touched the device
    with pytest.raises(ValueError, match="weighted"):
        s.fit(adata, fitting_kwargs={"weights_kl": np.ones(adata.n_obs)})
    # the same matrices are fine without resamples (a sweep of plain fits takes any non-negative X)
    sal.models.KLNMFSweep([2], max_iterations=10, min_iterations=10).fit(sal.AnnData(cases[0][0]))
    assert len(fakes.instances) == 1


def test_the_stand_alone_entry_validates_on_the_host():
    X = np.ones((3, 4))
    for bad, match in ((X * 0.5, "row 0"), (-X, "row 0"), (np.ones(4), "matrix")):
        with pytest.raises(ValueError, match=match):
            sal.resample_counts(bad, 2)
    with pytest.raises(ValueError, match="n_resamples"):
        sal.resample_counts(X, 0)
    with pytest.raises(ValueError, match="seed"):
        sal.resample_counts(X, 1, seed=-3)
    with pytest.raises(ValueError, match="columns"):
        sal.resample_counts(np.ones((2, 3073)), 1)
