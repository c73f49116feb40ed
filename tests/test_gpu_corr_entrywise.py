"""The dense pieces of CorrNMF on the device, entry by entry against the long double reference (``tests/_corr_ref.py``).

``test_gpu_corrnmf.py::test_dense_pieces_match_oracle`` compares whole matrices by rel-L2 on benign inputs; an exposure
or aux entry that is small and wrong in its leading digits is invisible to it.  Here EVERY entry of the exposures, both
scaling updates, aux, the signature update and the likelihood is compared in the unit that follows its own conditioning
(``_corr_ref`` docstring), at the shapes where each mechanism of ``corr_logit_mfma_kernel``, ``rowsum_X_kernel``,
``colsum_partial_kernel``, the aux pass (also blocked, V > 96) and forward mode 3 can go wrong, in five regimes:
(a) ordinary, (b) wide logits, (c) cancelling logits, (d) sparse counts, (e) P = 0 / subnormal in the likelihood.

Isolation: every operation is judged from the inputs the device itself had (aux from the downloaded H, beta from an
uploaded aux, ...), so errors do not compound.  Bounds: unit x ``_corr_ref.C``, C = 4 x the float64 oracle's own largest
ratio over the cases, measured on the CPU by ``test_corr_ref_host.py`` -- nothing here was tuned on the device.  The
device's ratios are printed (run with ``-s``); DESIGN.md section 8.1 records them.
"""

import numpy as np
import pytest

import _corr_ref as R
from salamander_amd import _lib
from salamander_amd.engine import Engine

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module", autouse=True)
def _release_cases():
    yield
    R.case.cache_clear()


def engine_from(X, W, beta, alpha, L, U):
    N, V = X.shape
    K, dim = L.shape
    e = Engine(N, V, K)
    e.upload_X(X)
    e.upload_W(W)
    e.corr_configure(dim)
    e.corr_upload(_lib.CORR_SIGNATURE_SCALINGS, beta)
    e.corr_upload(_lib.CORR_SAMPLE_SCALINGS, alpha)
    e.corr_upload(_lib.CORR_SIGNATURE_EMBEDDINGS, L)
    e.corr_upload(_lib.CORR_SAMPLE_EMBEDDINGS, U)
    return e


def _assert_within(name, tag, ratio, where):
    assert ratio <= R.C[name], f"{tag}: {name} at {where} is {ratio:.2f} units off, allowed {R.C[name]:.2f}"


@pytest.mark.parametrize("key", R.CASES, ids=lambda k: R.tag(*k))
def test_every_entry_in_its_unit(key):
    c = R.case(*key)
    tag = R.tag(*key)
    e = engine_from(c.X, c.W, c.beta, c.alpha, c.L, c.U)
    ratios = {}

    # alpha from (X, beta, L, U)
    e.corr_update_sample_scalings()
    alpha_dev = e.corr_download(_lib.CORR_SAMPLE_SCALINGS)
    ratios["alpha"] = R.abs_ratio(alpha_dev, c.alpha_new, c.alpha_unit)

    # H from (beta, alpha, L, U), the case's own alpha again
    e.corr_upload(_lib.CORR_SAMPLE_SCALINGS, c.alpha)
    e.corr_compute_exposures()
    H_dev = e.download_H()
    ratios["H"] = R.rel_ratio(H_dev, c.H, c.H_unit)

    # the likelihood of the resident (X, W, H_dev)
    llh_dev = e.corr_poisson_llh()
    llh, unit = R.poisson_llh(c.X, c.W, H_dev, c.gl)
    ratios["llh"] = (abs(float(R.LD(llh_dev) - llh)) / float(unit), ())

    # aux from the downloaded H; H is left alone
    e.corr_compute_aux()
    aux_dev = e.corr_download(_lib.CORR_AUX)  # (N, K)
    assert np.array_equal(e.download_H(), H_dev), f"{tag}: the aux pass changed H"
    aux = R.compute_aux(c.X, c.W, H_dev)  # (K, N)
    ratios["aux"] = R.rel_ratio(aux_dev.T, aux, R.aux_unit(c.K, c.V))

    # the signature update from the numerators of that pass
    e.corr_update_signatures(c.n_given)
    W_dev = e.download_W()
    new, raw = R.update_signatures(c.X, c.W, H_dev, c.n_given)
    assert np.array_equal(W_dev[: c.n_given], c.W[: c.n_given]), f"{tag}: given signatures changed"
    w = R.w_ratio(W_dev, new, raw, c.n_given, R.w_unit(c.N, c.K, c.V), R.C["W"])
    ratios["W"] = w[:2]
    if c.regime == "d" and c.n_given < c.K:
        assert w[2] >= c.K - c.n_given  # the feature nobody carries clips in every free signature

    # beta from an uploaded aux
    aux64 = np.ascontiguousarray(np.asarray(aux, dtype=np.float64).T)
    e.corr_upload(_lib.CORR_AUX, aux64)
    e.corr_update_signature_scalings()
    beta_dev = e.corr_download(_lib.CORR_SIGNATURE_SCALINGS)
    beta, unit = R.update_signature_scalings(aux64.T, c.alpha, c.L, c.U)
    ratios["beta"] = R.abs_ratio(beta_dev, beta, unit)
    e.close()

    print(f"\n[corr-entrywise] {tag}: device ratios " + "  ".join(f"{q} {ratios[q][0]:.3f}" for q in ("H", "alpha", "beta", "aux", "W", "llh"))
          + f"  (clipped entries of W: {w[2]})")
    for got in (alpha_dev, H_dev, aux_dev, W_dev, beta_dev):
        assert np.isfinite(got).all(), tag
    for q, (ratio, where) in ratios.items():
        _assert_within(q, tag, ratio, where)


@pytest.mark.parametrize("N,K,V", R.LLH_SHAPES)
def test_likelihood_where_P_is_zero_or_subnormal(N, K, V):
    """Regime (e): both branches of forward mode 3 (``_corr_ref.llh_states``); the reference counts 0 for ``x log p``
    where ``p == 0``."""
    X, states = R.llh_states(N, K, V)
    gl = R.gammaln_sums(X)
    e = Engine(N, V, K)
    e.upload_X(X)
    got = []
    for W, H in states:
        e.upload_W(W)
        e.upload_H(H)
        llh_dev = e.corr_poisson_llh()
        llh, unit = R.poisson_llh(X, W, H, gl)
        assert np.isfinite(llh_dev)
        got.append(abs(float(R.LD(llh_dev) - llh)) / float(unit))
    e.close()
    print(f"\n[corr-entrywise] (e) N={N} K={K} V={V}: device llh ratios " + "  ".join(f"{r:.4f}" for r in got))
    for i, r in enumerate(got):
        _assert_within("llh", f"(e) N={N} K={K} V={V} state {i}", r, ())


@pytest.mark.parametrize("regime", ["a", "b", "c"])
def test_a_row_subset_gives_the_same_bits(regime):
    """Pad rows and neighbours are not observable: 17 of the 65 samples alone (a ragged second tile instead of a fifth)
    give, bit for bit, the exposures and sample scalings they get inside the full run."""
    c = R.case(regime, 65, 5, 3, 96)
    rows = np.sort(np.random.default_rng(17).permutation(65)[:17])
    out = []
    for sel in (slice(None), rows):
        e = engine_from(c.X[sel], c.W, c.beta, c.alpha[sel], c.L, c.U[sel])
        e.corr_compute_exposures()
        H = e.download_H()
        e.corr_update_sample_scalings()
        out.append((H, e.corr_download(_lib.CORR_SAMPLE_SCALINGS)))
        e.close()
    (H_full, a_full), (H_part, a_part) = out
    assert np.array_equal(H_part, H_full[rows])
    assert np.array_equal(a_part, a_full[rows])
