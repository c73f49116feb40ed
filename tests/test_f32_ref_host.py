"""The fp32 fast mode's reference and error model on the CPU (``tests/_f32_ref.py``; the device: ``test_gpu_fast_entrywise.py``).

* ``exact_step`` is tied to the pinned oracle: on fp32-rounded inputs the two agree to fp64 rounding.
* A float32 NumPy replica of the step, in two summation orders, stays within the derived bounds ``E_H`` / ``E_W`` on every
  case the GPU file uses; the largest share of the bound it uses is recorded below -- the yardstick for the device's figures.
* The bound has teeth: six planted bugs each fail ``check`` on at least one case.
* The inputs are fit for the check: at most 1e-3 of a case's entries lie within the bound of EPSILON.
"""

import numpy as np
import pytest

import _f32_ref as fr
from oracle import klnmf_oracle as orc

# largest |replica - exact| / (bound * exact) over both orders and every case below, measured here (float32 NumPy on the
# host, deterministic): real fp32 arithmetic uses about a sixth of E_H and an eighth of E_W -- rounding errors of random
# sign add like sqrt(n), the bound adds them like n
REPLICA_MAX_H = 0.17  # measured 0.169 (one step; many tiles 0.145, chained 0.099, counts above 2^24 0.116)
REPLICA_MAX_W = 0.12  # measured 0.118 (one step; many tiles 0.017, chained 0.075, counts above 2^24 0.082)

CASES = fr.one_step_cases()
U64 = 2.0**-53


def _ids(c):
    return "K{}-N{}-V{}-g{}".format(*c)


def test_the_case_list_reaches_every_geometry():
    assert {K for K, _, _, _ in CASES} == set(fr.GEOMETRY_K) and {(N, V) for _, N, V, _ in CASES} == set(fr.SHAPES)
    assert {g for K, _, _, g in CASES if K == 64} == {0, 2} and {g for K, _, _, g in CASES if K == 1} == {0}
    floor = [c for c in CASES if fr.uses_floor_state(*c[:3])]
    assert len(floor) == 13 * 3 * 2  # every K >= 4 at the three shapes with more than one sample (asserted >= 25 % in case_state)
    assert fr.tiles_per_wave(39, 256) == 1 and fr.tiles_per_wave(fr.many_tiles_samples(256), 256) == 2
    assert fr.tiles_per_wave(fr.many_tiles_samples(64), 64) == 2 and fr.tiles_per_wave(16 * 1024, 256) == 1


@pytest.mark.parametrize("case", CASES[::3] + [(36, 39, 96, 0)], ids=_ids)
def test_exact_step_is_the_oracle_on_rounded_inputs(case):
    """fp64 against longdouble: the oracle's own rounding, the same model with ``u = 2^-53`` (G sums N samples)."""
    K, N, V, g = case
    X, W, H = (fr.rounded(a) for a in fr.case_state(*case))
    Hn, Wn, Hp, Wp = fr.exact_step(X, W, H, g)
    Wo, Ho = (a.T for a in orc.update_WH(X.T, W.T, H.T, None, None, g))
    assert fr.check(Ho, Hn, Hp, (K + V + 8) * U64, f"{case}/H") <= 1.0
    assert fr.check(Wo, Wn, Wp, 2 * (K + N + 8) * U64, f"{case}/W") <= 1.0
    assert np.array_equal(Wo[:g], W[:g]) and np.array_equal(Wn[:g], W[:g])


def test_exact_step_rounds_the_inputs_but_not_w_in_the_tail():
    K, N, V, g = 9, 39, 83, 2
    X, W, H = fr.case_state(K, N, V, g)
    assert (fr.rounded(W) != W).any() and (fr.rounded(H) != H).any()
    a = fr.exact_step(X, W, H, g)
    b = fr.exact_step(fr.rounded(X), W, fr.rounded(H), g)
    assert all(np.array_equal(x, y) for x, y in zip(a, b))
    # W' = W * G / sum: the tail multiplies the fp64 W
    G = (a[3] / W)[g:]  # proportional to G row by row
    c = fr.exact_step(X, fr.rounded(W), H, g)
    assert not np.array_equal(a[3][g:], c[3][g:])
    assert np.allclose(G / G.sum(axis=1, keepdims=True), (c[3] / fr.rounded(W))[g:] / (c[3] / fr.rounded(W))[g:].sum(axis=1, keepdims=True), rtol=1e-12)
    assert np.array_equal(a[1][:g], W[:g])  # given rows: the input's bits
    # every signature given: W untouched
    d = fr.exact_step(X, W, H, K)
    assert np.array_equal(d[1], W) and np.array_equal(d[0], a[0])


def _replica_ratios(X, W, H, g, K, V, T_w, cus, what):
    Hn, Wn, Hp, Wp = fr.exact_step(X, W, H, g)
    fr.assert_no_underflow(X, W, H)
    rh = rw = 0.0
    for order in (0, 1):
        h, w = fr.replica_step(X, W, H, g, order, cus=cus)
        rh = max(rh, fr.check(h, Hn, Hp, fr.bound_H(K, V), f"{what}/H/order{order}"))
        rw = max(rw, fr.check(w, Wn, Wp, fr.bound_W(K, T_w), f"{what}/W/order{order}"))
        assert np.array_equal(w[:g], W[:g]) and (h >= fr.EPS).all() and np.array_equal(fr.rounded(h), h)
    return rh, rw


def test_replica_within_the_bound_one_step_every_geometry():
    rh = rw = 0.0
    for case in CASES:
        K, N, V, g = case
        X, W, H = fr.case_state(*case)
        Hn, Wn, Hp, Wp = fr.case_exact(*case)
        fr.assert_no_underflow(X, W, H)
        for order in (0, 1):
            h, w = fr.replica_step(X, W, H, g, order)
            rh = max(rh, fr.check(h, Hn, Hp, fr.bound_H(K, V), f"{case}/H/order{order}"))
            rw = max(rw, fr.check(w, Wn, Wp, fr.bound_W(K, 1), f"{case}/W/order{order}"))
            assert np.array_equal(w[:g], W[:g])
    print(f"F32REPLICA one-step H {rh:.3f} W {rw:.3f}")
    assert rh <= REPLICA_MAX_H and rw <= REPLICA_MAX_W


@pytest.mark.parametrize("K", fr.MANY_TILES_K)
def test_replica_within_the_bound_more_tiles_than_waves(K):
    cus = fr.MI355X_CUS
    X, W, H = fr.many_tiles_state(K, cus)
    rh, rw = _replica_ratios(X, W, H, 0, K, fr.VMAX, 2, cus, f"many{K}")
    print(f"F32REPLICA many-tiles K={K} H {rh:.3f} W {rw:.3f}")
    assert rh <= REPLICA_MAX_H and rw <= REPLICA_MAX_W


@pytest.mark.parametrize("K", fr.CHAINED_K)
def test_replica_within_the_bound_five_chained_steps(K):
    X, W, H = fr.case_state(K, 39, 96, 0)
    rh = rw = 0.0
    for step in range(5):
        a, b = _replica_ratios(X, W, H, 0, K, 96, 1, 256, f"chain{K}/step{step}")
        rh, rw = max(rh, a), max(rw, b)
        H, W = fr.replica_step(X, W, H, 0, step & 1)
    print(f"F32REPLICA chained K={K} H {rh:.3f} W {rw:.3f}")
    assert rh <= REPLICA_MAX_H and rw <= REPLICA_MAX_W


def test_replica_within_the_bound_counts_above_2_to_24():
    X, W, H = fr.big_counts_state()
    K, V = W.shape
    rh, rw = _replica_ratios(X, W, H, 0, K, V, 1, 256, "big")
    print(f"F32REPLICA big-counts H {rh:.3f} W {rw:.3f}")
    assert rh <= REPLICA_MAX_H and rw <= REPLICA_MAX_W
    # against the fp64 oracle on the unrounded X: W and H are fp32 numbers already, rounding X moves R by u, so H' by u
    # and W' (a quotient of two sums of R) by 2 u
    Hn, Wn, Hp, Wp = fr.exact_step(X, W, H, 0)
    Wo, Ho = (a.T for a in orc.update_WH(X.T, W.T, H.T))
    assert fr.check(Hn, Ho, Hp, 2 * fr.U32, "big/exact-oracle/H") <= 1.0 and fr.check(Wn, Wo, Wp, 2 * fr.U32, "big/exact-oracle/W") <= 1.0
    assert np.abs(Hn - Ho).max() > 0  # the rounding of X is visible at all


# ------------------------------------------------------------------ the bound has teeth


def _fails(dev, exact, pre, bound):
    try:
        fr.check(dev, exact, pre, bound)
    except AssertionError:
        return True
    return False


def _caught(mutate, cases):
    """The cases on which the planted bug fails ``check`` (H or W), over both orders."""
    hit = []
    for case in cases:
        K, N, V, g = case
        X, W, H = fr.case_state(*case)
        Hn, Wn, Hp, Wp = fr.case_exact(*case)
        for order in (0, 1):
            with np.errstate(all="ignore"):
                h, w = fr.replica_step(X, W, H, g, order, mutate=mutate)
            if _fails(h, Hn, Hp, fr.bound_H(K, V)) or _fails(w, Wn, Wp, fr.bound_W(K, 1)):
                hit.append((case, order))
    return hit


@pytest.mark.parametrize("mutate", ["u_last_feature", "g_sample15", "floor0", "p_drop"])
def test_a_planted_bug_fails_the_check(mutate):
    """(a) the last real feature left out of U, (b) sample 15 of a tile left out of G, (d) the floor written as 0, (f) one
    signature beyond a multiple of 4 dropped from P."""
    cases = [c for c in CASES if mutate != "p_drop" or c[0] % 4]
    if mutate == "g_sample15":
        cases = [c for c in cases if c[1] >= 16]  # (a tile that has a sample 15)
    hit = _caught(mutate, cases)
    print(f"F32MUTANT {mutate}: caught on {len(hit)} of {2 * len(cases)} runs")
    assert hit
    if mutate == "p_drop":  # wrong on every such case, in either order
        assert len(hit) == 2 * len(cases)
    if mutate == "floor0":  # wrong wherever H has a floor at all
        assert {c for c, _ in hit} >= {c for c in cases if fr.uses_floor_state(*c[:3])}


def test_pad_columns_of_w_at_zero_give_nan_below_96_features():
    """(e): with V < 96 the pad features have X = 0 and must have P > 0; a pad of 0 makes R = 0 * inf there."""
    narrow = [c for c in CASES if c[2] < fr.VMAX]
    assert len(_caught("wpad0", narrow)) == 2 * len(narrow)
    assert not _caught("wpad0", [c for c in CASES if c[2] == fr.VMAX][:8])  # nothing to pad, nothing planted


def test_a_stale_shadow_of_h_fails_the_check():
    """(c): the second step reads the fp32 copy of H that the first one started from."""
    hit = 0
    for K in fr.CHAINED_K:
        X, W, H0 = fr.case_state(K, 39, 96, 0)
        H1, W1 = fr.replica_step(X, W, H0, 0, 0)
        Hn, Wn, Hp, Wp = fr.exact_step(X, W1, H1, 0)
        h, w = fr.replica_step(X, W1, H1, 0, 0, mutate="stale", stale_H=H0)
        hit += _fails(h, Hn, Hp, fr.bound_H(K, 96)) or _fails(w, Wn, Wp, fr.bound_W(K, 1))
        h, w = fr.replica_step(X, W1, H1, 0, 0)  # and the honest second step passes
        assert not _fails(h, Hn, Hp, fr.bound_H(K, 96)) and not _fails(w, Wn, Wp, fr.bound_W(K, 1))
    assert hit == len(fr.CHAINED_K)


# ------------------------------------------------------------------ conditions on the inputs


def test_few_entries_lie_within_the_bound_of_the_floor():
    """With the reference alone: the share of entries that may come back as either value is at most 1e-3 per case."""
    worst = 0.0
    states = [(fr.case_exact(*c), c[0], c[2], 1) for c in CASES]
    states += [(fr.exact_step(*fr.many_tiles_state(K, fr.MI355X_CUS), 0), K, 96, 2) for K in fr.MANY_TILES_K]
    states += [(fr.exact_step(*fr.big_counts_state(), 0), 12, 96, 1)]
    for (Hn, Wn, Hp, Wp), K, V, T_w in states:
        sh, sw = fr.ambiguous_share(Hp, fr.bound_H(K, V)), fr.ambiguous_share(Wp, fr.bound_W(K, T_w))
        worst = max(worst, sh, sw)
        assert sh <= fr.AMBIGUOUS_SHARE and sw <= fr.AMBIGUOUS_SHARE, (K, V, sh, sw)
    print(f"F32AMBIGUOUS worst share {worst:.2e}")


def test_check_itself():
    fill = np.linspace(1.0, 2.0, 2000)  # (so that the two entries next to the floor stay below the ambiguous share)
    exact = np.concatenate([[1.0, fr.EPS, fr.EPS, 3.0], fill])
    pre = np.concatenate([[1.0, fr.EPS * 0.5, fr.EPS * (1 - 1e-7), 3.0], fill])
    dev = lambda *head: np.concatenate([head, fill])
    b = 1e-6
    assert fr.check(dev(1.0 + 5e-7, fr.EPS, fr.EPS * (1 + 2e-7), 3.0), exact, pre, b) == pytest.approx(0.5)
    for head in ([1.0 + 2e-6, fr.EPS, fr.EPS, 3.0], [1.0, fr.EPS * (1 + 1e-7), fr.EPS, 3.0], [1.0, 0.0, fr.EPS, 3.0], [1.0, fr.EPS, fr.EPS, np.nan], [1.0, fr.EPS, fr.EPS, np.inf]):
        assert _fails(dev(*head), exact, pre, b), head
    nan = dev(1.0, fr.EPS, fr.EPS, np.nan)
    assert fr.check(nan, nan, nan, b) == 0.0
    # too many entries next to the floor: the inputs, not the device, are at fault -- still an error
    near = np.full(100, fr.EPS * (1 + 1e-7))
    assert _fails(near, near, near, b)
