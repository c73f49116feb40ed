"""KLNMFSweep with a penalty axis and shared KL weights on the MI355X: every member bit for bit the single weighted fit
(``KLNMF.fit(..., fitting_kwargs={"weights_kl": w, "weights_lhalf": penalty})``, which runs the per-step weighted path)."""
import os

import numpy as np
import pytest

import salamander_amd as sal
from conftest import GOLDEN, read_counts

pytestmark = pytest.mark.gpu

SETTINGS = dict(init_method="random", min_iterations=30, max_iterations=97, tol=1e-4)
LAM = 2.0  # an l-half weight of the order of sqrt(exposure) / KL gradient on this catalogue: it moves the exposures (asserted)


@pytest.fixture(scope="module")
def pcawg():
    return sal.AnnData(read_counts(os.path.join(GOLDEN, "pcawg_breast_sbs.csv")).T)


@pytest.fixture(scope="module")
def wkl(pcawg):
    return np.random.default_rng(11).uniform(0.5, 2.0, pcawg.X.shape[0])


def single(X, K, seed, w, lam):
    m = sal.models.KLNMF(K, objective_in_step=False, **SETTINGS)
    m.fit(sal.AnnData(np.array(X, copy=True)), None, {"seed": seed}, {"weights_kl": w, "weights_lhalf": lam})
    m.compute_reconstruction_errors()
    m._engine.close()
    return m


def assert_same(got, ref):
    assert got.n_iterations_ == ref.n_iterations_
    assert got.history["objective_function"] == ref.history["objective_function"]
    assert np.array_equal(got.asignatures.X, ref.asignatures.X)
    assert np.array_equal(got.adata.obsm["exposures"], ref.adata.obsm["exposures"])
    assert np.array_equal(np.asarray(got.adata.obs["reconstruction_error"]), np.asarray(ref.adata.obs["reconstruction_error"]))


@pytest.mark.parametrize("F", [0, 2])
def test_penalty_sweep_members_equal_single_fits(pcawg, wkl, F):
    Ks, seeds, lams = [2, 5, 9], [0, 1], [0.0, LAM]
    s = sal.models.KLNMFSweep(Ks, seeds=seeds, lhalf_weights=lams, weights_kl=wkl, n_splits=F, **SETTINGS)
    models = s.fit(pcawg)
    assert s.batched_.all() and len(models) == 12 * max(1, F)
    order = [(K, l, sd, f) for K in Ks for l in range(2) for sd in seeds for f in range(max(1, F))]
    assert list(s.lhalf_of_) == [o[1] for o in order]
    for got, (K, l, sd, f) in zip(models, order):
        X = s.train_splits_[f] if F else pcawg.X
        assert_same(got, single(X, K, sd, wkl, lams[l]))
    shape = (3, 2, 2) + ((F,) if F else ())
    assert s.reconstruction_errors_.shape == shape
    if F:
        assert np.array_equal(s.heldout_errors_.reshape(-1), [float(np.sum(np.asarray(m.adata.obs["heldout_error"]))) for m in models])
        assert s.heldout_mean_.shape == (3, 2) and s.suggest_penalty_heldout()[0] in Ks
    # the penalty moves the exposures: member (K, LAM, seed) against (K, 0.0, seed)
    per = 2 * max(1, F)
    assert not np.array_equal(models[0].adata.obsm["exposures"], models[per].adata.obsm["exposures"])


def test_a_member_out_of_reach_takes_the_single_weighted_fit(pcawg, wkl):
    s = sal.models.KLNMFSweep([2, 17], seeds=[0], lhalf_weights=[LAM], weights_kl=wkl, **SETTINGS)
    models = s.fit(pcawg)
    assert list(s.batched_) == [True, False]
    for got, K in zip(models, [2, 17]):
        assert_same(got, single(pcawg.X, K, 0, wkl, LAM))
