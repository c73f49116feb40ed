"""The oracle on the EPSILON clip floor, pinned entry by entry to the reference (``tests/golden/kl_floor.npz``).

CPU only.  The fixture was written by ``tests/golden/make_golden.py --floor`` from the reference's own functions on a
sparse catalogue where about half of W and H sit at the floor, with given signatures that hold entries below it (0,
1e-12, 1e-9) and a channel that is 0 in every given signature.  The GPU tests (``test_gpu_floor.py``) compare the device
with the oracle, so the floor semantics they check rest on this file.
"""

import os

import numpy as np
import pytest

from _floor import EPS, assert_entrywise, floor_share, lhalf_allowance
from conftest import GOLDEN
from oracle import klnmf_oracle as orc

# the oracle restates the reference's NumPy expressions; only the order of a few products differs
RTOL = 1e-13


@pytest.fixture(scope="module")
def fl():
    return np.load(os.path.join(GOLDEN, "kl_floor.npz"))


def test_fixture_sits_on_the_floor(fl):
    g = int(fl["n_given"])
    assert floor_share(fl["H"]) >= 0.25 and floor_share(fl["W"]) >= 0.25
    assert floor_share(fl["X"]) >= 0.5
    Wg = fl["W"][:, :g]
    assert (Wg == 0).any() and (Wg == 1e-12).any() and (Wg == 1e-9).any()
    # the next step clips: without that the fixture could not tell a missing clip from a present one
    Wp, Hp, _, _ = orc.update_WH_preclip(fl["X"], fl["W"], fl["H"])
    assert np.mean(Hp < EPS) >= 0.25 and np.mean(Wp < EPS) >= 0.25
    _, Hp, _, _ = orc.update_WH_preclip(fl["X"], fl["W"], fl["H"], fl["wkl"], fl["wlh"], g)
    assert np.mean(Hp < EPS) >= 0.25


@pytest.mark.parametrize("tag,ng", [("g0", 0), ("g3", 3), ("gK", 8)])
def test_update_WH_entrywise(fl, tag, ng):
    X, W, H = fl["X"], fl["W"], fl["H"]
    Wn, Hn = orc.update_WH(X, W, H, None, None, ng)
    Wp, Hp, _, _ = orc.update_WH_preclip(X, W, H, None, None, ng)
    assert_entrywise(Hn, fl[f"WH_{tag}_H"], RTOL, pre=Hp, what="H")
    if ng == W.shape[1]:
        # all given: W untouched, not even clipped (:330-331)
        assert np.array_equal(fl[f"WH_{tag}_W"], W) and np.array_equal(Wn, W)
        return
    assert_entrywise(Wn, fl[f"WH_{tag}_W"], RTOL, pre=Wp, what="W")
    if ng:
        # the joint step clips the given columns too (:338-341): the zeros and 1e-12 / 1e-9 become EPSILON
        assert np.array_equal(fl[f"WH_{tag}_W"][:, :ng], W[:, :ng].clip(EPS))
        assert not np.array_equal(W[:, :ng].clip(EPS), W[:, :ng])


def test_update_WH_lhalf_entrywise(fl):
    X, W, H, wkl, wlh, g = fl["X"], fl["W"], fl["H"], fl["wkl"], fl["wlh"], int(fl["n_given"])
    Wn, Hn = orc.update_WH(X, W, H, wkl, wlh, g)
    Wp, Hp, t, disc = orc.update_WH_preclip(X, W, H, wkl, wlh, g)
    assert_entrywise(Wn, fl["WH_lh_W"], RTOL, pre=Wp, what="W")
    assert_entrywise(Hn, fl["WH_lh_H"], RTOL, pre=Hp, allowance=lhalf_allowance(t, disc, wkl), what="H")
    assert np.array_equal(Hn, _clip(Hp))  # the pre-clip helper is the update before its clip


def _clip(a):
    return np.clip(a, EPS, None)


def test_update_W_keeps_given_columns_bit_for_bit(fl):
    X, W, H, wkl, g = fl["X"], fl["W"], fl["H"], fl["wkl"], int(fl["n_given"])
    for want, wk, ng in ((fl["W_g0"], None, 0), (fl["W_g3"], None, g), (fl["W_g3_wkl"], wkl, g)):
        got = orc.update_W(X, W, H, wk, ng)
        Wp, _, _, _ = orc.update_WH_preclip(X, W, H, wk, None, ng)
        assert_entrywise(got[:, ng:], want[:, ng:], RTOL, pre=Wp[:, ng:], what="W free")
        # update_W clips only the free columns (:215): the given ones come back as they went in, zeros included
        assert np.array_equal(want[:, :ng], W[:, :ng]) and np.array_equal(got[:, :ng], W[:, :ng])


def test_update_H_entrywise(fl):
    X, W, H, wkl, wlh = fl["X"], fl["W"], fl["H"], fl["wkl"], fl["wlh"]
    _, Hp, _, _ = orc.update_WH_preclip(X, W, H)
    assert_entrywise(orc.update_H(X, W, H), fl["H_plain"], RTOL, pre=Hp, what="H")
    for want, wk in ((fl["H_lh"], wkl), (fl["H_lh_nokl"], None)):
        _, Hp, t, disc = orc.update_WH_preclip(X, W, H, wk, wlh)
        assert_entrywise(orc.update_H(X, W, H, wk, wlh), want, RTOL, pre=Hp, allowance=lhalf_allowance(t, disc, wk), what="H l-half")


def test_objectives_on_the_floor(fl):
    X, W, H, wkl = fl["X"], fl["W"], fl["H"], fl["wkl"]
    assert np.isclose(orc.kl_divergence(X, W, H), fl["kl"], rtol=1e-13, atol=0)
    assert np.isclose(orc.kl_divergence(X, W, H, wkl), fl["kl_w"], rtol=1e-13, atol=0)
    assert np.allclose(orc.samplewise_kl_divergence(X, W, H), fl["skl"], rtol=1e-12, atol=1e-12)


@pytest.mark.parametrize("tag,ng", [("g0", 0), ("g3", 3)])
def test_mvnmf_step_entrywise(fl, tag, ng):
    X, W, H = fl["X"], fl["W"], fl["H"]
    lam, delta = fl["mv_par"]
    Hm = orc.update_H(X, W, H)
    assert_entrywise(Hm, fl[f"mv_{tag}_H"], RTOL, what="H")
    Wu = orc.update_W_unconstrained(X, W, fl[f"mv_{tag}_H"], lam, delta, ng)
    assert_entrywise(Wu[:, ng:], fl[f"mv_{tag}_Wunc"][:, ng:], 1e-12, what="W unconstrained")
    assert np.array_equal(Wu[:, :ng], W[:, :ng])
    Wn, Hn, gamma = orc.line_search(X, W, fl[f"mv_{tag}_H"], lam, delta, 1.0, fl[f"mv_{tag}_Wunc"])
    assert gamma == fl[f"mv_{tag}_gamma"]
    assert_entrywise(Wn, fl[f"mv_{tag}_W"], 1e-12, what="W")
    assert_entrywise(Hn, fl[f"mv_{tag}_Hn"], 1e-12, what="H rescaled")
    Wn2, Hn2, gamma2 = orc.mvnmf_step(X, W, H, lam, delta, 1.0, ng)
    assert gamma2 == gamma and np.allclose(Wn2, Wn, rtol=1e-12, atol=0) and np.allclose(Hn2, Hn, rtol=1e-12, atol=0)


def test_zero_model_channel_gives_the_references_inf_nan_pattern(fl):
    """Every signature given, channel 0 is 0 in all of them: P = 0 there.  0/0 and x/0 reach the divergences and H."""
    Xz, Wz, H = fl["Xz"], fl["Wz"], fl["H"]
    K = Wz.shape[1]
    with np.errstate(divide="ignore", invalid="ignore"):
        kl = orc.kl_divergence(Xz, Wz, H)
        skl = orc.samplewise_kl_divergence(Xz, Wz, H)
        Wn, Hn = orc.update_WH(Xz, Wz, H, None, None, K)
        Hh = orc.update_H(Xz, Wz, H)
    assert kl == fl["z_kl"] == np.inf
    assert np.array_equal(np.isinf(skl), np.isinf(fl["z_skl"])) and np.isinf(skl).any() and np.isfinite(skl).any()
    fin = np.isfinite(skl)
    assert np.allclose(skl[fin], fl["z_skl"][fin], rtol=1e-12, atol=1e-12)
    assert np.array_equal(Wn, fl["z_WH_W"]) and np.array_equal(Wn, Wz)
    for got, want in ((Hn, fl["z_WH_H"]), (Hh, fl["z_H"])):
        assert np.array_equal(np.isnan(got), np.isnan(want)) and np.array_equal(np.isinf(got), np.isinf(want))


# ------------------------------------------------------------------ the generator and the comparison themselves


def test_sparse_problem_shape_of_the_data():
    X, W0, H0 = orc.sparse_problem(96, 1000, 20, seed=0)
    assert X.shape == (1000, 96) and W0.shape == (20, 96) and H0.shape == (1000, 20)
    assert 0.6 <= floor_share(X) <= 0.7  # ~65 % of a 96-channel catalogue is unobserved
    assert (X.max(axis=1) == EPS).sum() >= 1 and (X.max(axis=0) == EPS).sum() >= 1  # all-zero samples, dead channels
    counts = np.where(X == EPS, 0.0, X).sum(axis=1)
    assert (X >= EPS).all() and 150 <= np.median(counts) <= 260 and counts.max() <= 550  # 20-400 mutations (Poisson)
    Xw, _, _ = orc.sparse_problem(1536, 200, 10, seed=0)
    assert 0.85 <= floor_share(Xw) <= 0.95  # SBS-1536
    X2, W2, H2 = orc.floor_state(96, 1000, 20, seed=0)
    assert floor_share(H2) >= 0.25 and floor_share(W2) >= 0.25


def test_assert_entrywise_bites():
    X, W, H = orc.floor_state(96, 300, 12, seed=3)
    Wn, Hn = orc.update_WH(X.T, W.T, H.T)
    Wp, Hp, _, _ = orc.update_WH_preclip(X.T, W.T, H.T)
    assert assert_entrywise(Hn, Hn, 0.0, pre=Hp) == 0.0
    below = Hp < EPS
    assert below.mean() >= 0.25
    for broken in (np.where(below, 0.0, Hn), np.where(below, Hp, Hn), Hn * (1 + 1e-12)):
        with pytest.raises(AssertionError):
            assert_entrywise(broken, Hn, 1e-13, pre=Hp)
    nan = Hn.copy()
    nan[0, 0] = np.nan
    with pytest.raises(AssertionError, match="NaN"):
        assert_entrywise(nan, Hn, 1.0)
    # the floor kept exactly, everything else within rtol: passes
    assert assert_entrywise(np.where(Wn == EPS, EPS, Wn * (1 + 1e-14)), Wn, 1e-13, pre=Wp) < 1e-13
