"""The inputs of ``test_gpu_pending_scale.py`` (``tests/_scale_ref.py``) are not vacuous: conditions on the inputs, checked
on the host so that the GPU file never computes one itself.

Per case: at least 5 % of ``H0 * scale`` lies below EPSILON before the clip (a missing clip writes values below the
floor), at least 5 % of H0's floor entries leave the floor, no scale entry within 10 % of 1, and the oracle's objectives
of the materialised, the unscaled and the twice-scaled state differ pairwise by more than 1 % ("not applied" and "applied
twice" are both far outside every tolerance).  The MvNMF states: the accepted ones accept and the backtracking one
backtracks under ``orc.mvnmf_step``.  Run with ``-s`` for the figures.
"""

import numpy as np
import pytest

import _scale_ref as S
from oracle import klnmf_oracle as orc

CASES = S.all_cases() + S.all_cases([S.COOP_SHAPE])


@pytest.mark.parametrize("p", CASES, ids=S.case_id)
def test_case_conditions(p):
    c = S.case(*p)
    K = c.K
    assert c.X.shape == (c.N, c.V) and c.W.shape == (K, c.V) and c.H0.shape == (c.N, K)
    # ragged N; the cooperative case is 1024 + 1 tiles exactly (one leftover tile on a 256-CU grid of four waves each)
    assert c.N % 16 != 0 or p[:3] == S.COOP_SHAPE
    assert (c.H0 >= S.EPS).all() and np.mean(c.H0 == S.EPS) >= 0.05, "H0 has no share at the floor"
    for s in (c.scale, c.scale2):
        assert s.shape == (K,) and (np.abs(s - 1.0) > 0.1).all()
        if K > 1:
            assert (s == S.TINY).sum() >= 1 and (s >= 2.0).sum() >= 1
            rest = s[s != S.TINY]
            assert ((rest >= 0.2) & (rest <= 3.0)).all()
    assert np.array_equal(c.Hs, np.clip(c.H0 * c.scale[None, :], S.EPS, None)) and (c.Hs >= S.EPS).all()
    clipped, lifted, f = c.conditions()
    sep = S.separation(f)
    print(f"\n[scale-ref] {c.tag}: clipped {clipped:.3f} lifted {lifted:.3f} objectives Hs {f[0]:.6g} H0 {f[1]:.6g} twice {f[2]:.6g} separation {sep:.3g}")
    if c.variant != "up":
        assert clipped >= 0.05, clipped
    if c.variant != "down":
        assert lifted >= 0.05, lifted
    assert all(np.isfinite(f)) and sep > 0.01, (f, sep)


@pytest.mark.parametrize("p", S.all_cases(), ids=S.case_id)
def test_composition_rule(p):
    """``set_H_scale(s1); set_H_scale(s2)`` reads as ``clip(clip(H0 s1) s2)``: not the same as the product of the scales
    under one clip wherever the first clip acted, so a reader that merged the two scales is visible."""
    c = S.case(*p)
    two = S.compose(c.H0, c.scale, c.scale2)
    assert np.array_equal(two, np.clip(np.clip(c.H0 * c.scale, S.EPS, None) * c.scale2, S.EPS, None))
    merged = np.clip(c.H0 * (c.scale * c.scale2), S.EPS, None)
    if c.K > 1:
        assert np.mean(two != merged) >= 0.01, "the order of clip and scale does not show in this case"
    f2 = orc.kl_divergence(c.X.T, c.W.T, two.T)
    f1 = orc.kl_divergence(c.X.T, c.W.T, c.Hs.T)
    assert abs(f2 - f1) > 0.01 * max(abs(f1), abs(f2)), (f1, f2)


@pytest.mark.parametrize("name", S.MV_CASES)
def test_mvnmf_states_accept_and_backtrack(name):
    m = S.mv_case(name)
    V, N, K = m.shape
    Wn, Hn, gamma = orc.mvnmf_step(m.X.T, m.W.T, m.H.T, m.lam, m.delta, 1.0, m.n_given)
    # (the stored step ran on other array layouts: BLAS may round its products differently)
    assert gamma == m.gamma and np.allclose(Wn.T, m.Wn, rtol=1e-9, atol=0) and np.allclose(Hn.T, m.Hn, rtol=1e-9, atol=0)
    print(f"\n[scale-ref] mv {name}: {V}x{N}x{K} lam {m.lam:g} gamma {gamma!r}")
    if name == "backtracking":
        assert V <= 96 and K <= 64 and m.backtracks and gamma < 1.0, gamma
    else:
        assert gamma == 1.0 and not m.backtracks, gamma
    assert (name in S.MV_CHUNKED) == (K > 64)
    # the rescale the accepted trial leaves pending is not the identity: the exposures after the step are not update_H's
    H1 = orc.update_H(m.X.T, m.W.T, m.H.T).T
    moved = float(np.mean(np.abs(m.Hn - H1) > 1e-6 * H1))
    print(f"[scale-ref] mv {name}: share of exposures the pending rescale moves by more than 1e-6: {moved:.3f}")
    assert moved >= 0.05, moved
