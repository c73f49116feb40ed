"""The fp32 fast mode (``fused_f32_kernel<KS>``, ``kl_steps_f32``) entry by entry, from the shadow copies to the hand-back.

Every comparison is either bit for bit (``np.array_equal``) or against ``_f32_ref.exact_step`` -- the mode's step in
extended precision on the fp32-rounded inputs -- within the bounds ``E_H = (K + V + 8) u`` and ``E_W = 2 (K + 16 T_w + 8) u``
derived in ``tests/_f32_ref.py`` (``u = 2^-24``).  No tolerance here was read off a device; ``test_f32_ref_host.py`` shows
on the CPU that float32 arithmetic uses a fifth of these bounds at most and that six planted bugs exceed them.

Run with ``-s``: each group prints the largest error / bound it saw (``F32MAX``).
"""

import numpy as np
import pytest

import _f32_ref as fr
from oracle import klnmf_oracle as orc
from salamander_amd import Engine

pytestmark = pytest.mark.gpu

EPS = fr.EPS


def _cus():
    import torch  # (about ten seconds where nothing has imported it yet; the suite has, long before this file)

    return int(torch.cuda.get_device_properties(0).multi_processor_count)


def engine(X, W, H, precision="f32", small_tiles=None):
    N, V = X.shape
    e = Engine(N, V, W.shape[0])
    if small_tiles is not None:
        e.set_small_cohort_tiles(small_tiles)
    e.upload_X(X), e.upload_W(W), e.upload_H(H)
    e.set_precision(precision)
    return e


def state_of(e):
    return e.download_W(), e.download_H()


def same_state(a, b):
    return all(np.array_equal(x, y) for x, y in zip(state_of(a), state_of(b)))


def check_step(tag, Wd, Hd, X, W, H, g, T_w=1, exact=None):
    """The device's ``(Wd, Hd)`` after one fp32 step from ``(W, H)``: ``(worst H, worst W)`` as shares of the bounds."""
    K, V = W.shape
    Hn, Wn, Hp, Wp = exact if exact is not None else fr.exact_step(X, W, H, g)
    fin = np.isfinite(Hd)
    assert np.array_equal(fr.rounded(Hd[fin]), Hd[fin]) and (Hd[fin] >= EPS).all(), f"{tag}: H is not a clipped fp32 array"
    rh = fr.check(Hd, Hn, Hp, fr.bound_H(K, V), f"{tag}/H")
    rw = fr.check(Wd, Wn, Wp, fr.bound_W(K, T_w), f"{tag}/W")
    assert np.array_equal(Wd[:g], W[:g]), f"{tag}: given rows of W moved"
    return rh, rw


def _report(group, rh, rw):
    print(f"F32MAX {group} H {rh:.3f} W {rw:.3f}")


# ------------------------------------------------------------------ one step, every geometry


@pytest.mark.parametrize("K", fr.GEOMETRY_K)
def test_one_step_every_geometry(K):
    """Both ends of every KS; three tiles with a ragged last one, V < 96, one full tile, one sample; with and without given
    signatures.  States with a quarter of H at the floor wherever the shape allows one (asserted in ``case_state``)."""
    rh = rw = 0.0
    cases = [c for c in fr.one_step_cases() if c[0] == K]
    assert len(cases) == (4 if K == 1 else 8)
    for case in cases:
        _, N, V, g = case
        X, W, H = fr.case_state(*case)
        e = engine(X, W, H)
        e.kl_step(1, g)
        Wd, Hd = state_of(e)
        e.close()
        a, b = check_step("K{}-N{}-V{}-g{}".format(*case), Wd, Hd, X, W, H, g, exact=fr.case_exact(*case))
        rh, rw = max(rh, a), max(rw, b)
    _report(f"one-step K={K}", rh, rw)


@pytest.mark.parametrize("K", fr.MANY_TILES_K)
def test_more_tiles_than_waves(K):
    """Every wave of the grid takes one tile and some a second one: two tiles' samples add up in fp32 (``T_w = 2``)."""
    cus = _cus()
    N = fr.many_tiles_samples(cus)
    assert fr.tiles_per_wave(N, cus) == 2
    X, W, H = fr.many_tiles_state(K, cus)
    e = engine(X, W, H)
    e.kl_step(1, 0)
    Wd, Hd = state_of(e)
    e.close()
    _report(f"many-tiles K={K} N={N}", *check_step(f"many{K}", Wd, Hd, X, W, H, 0, T_w=2))


# ------------------------------------------------------------------ steps chained without compounding


@pytest.mark.parametrize("K", fr.CHAINED_K)
def test_five_single_steps_each_within_the_bound_and_equal_to_one_call_of_five(K):
    X, W, H = fr.case_state(K, 39, 96, 0)
    e = engine(X, W, H)
    rh = rw = 0.0
    for step in range(5):
        e.kl_step(1, 0)
        Wd, Hd = state_of(e)
        a, b = check_step(f"chain{K}/step{step}", Wd, Hd, X, W, H, 0)
        rh, rw = max(rh, a), max(rw, b)
        W, H = Wd, Hd
    _report(f"chained K={K}", rh, rw)
    five = engine(*fr.case_state(K, 39, 96, 0))
    five.kl_step(5, 0)  # float -> double -> float between the calls is exact
    assert same_state(e, five)
    e.close(), five.close()


# ------------------------------------------------------------------ counts above 2^24


def test_counts_above_2_to_24():
    X, W, H = fr.big_counts_state()
    assert all((X == c).any() for c in fr.BIG_COUNTS)
    e = engine(X, W, H)
    e.kl_step(1, 0)
    Wd, Hd = state_of(e)
    e.close()
    _report("big-counts", *check_step("big", Wd, Hd, X, W, H, 0))
    # the fp64 oracle on the unrounded X: W and H are fp32 numbers, so X is the only input the shadow copies round --
    # u on R, so u on H' and 2 u on W' (a quotient of two sums over R): E + 2 u
    K, V = W.shape
    Wo, Ho = (a.T for a in orc.update_WH(X.T, W.T, H.T))
    Wp, Hp, _, _ = orc.update_WH_preclip(X.T, W.T, H.T)
    rh = fr.check(Hd, Ho, Hp.T, fr.bound_H(K, V) + 2 * fr.U32, "big/oracle/H")
    rw = fr.check(Wd, Wo, Wp.T, fr.bound_W(K, 1) + 2 * fr.U32, "big/oracle/W")
    _report("big-counts vs fp64 oracle", rh, rw)


# ------------------------------------------------------------------ rows do not meet in H


@pytest.mark.parametrize("K", [12, 36])
def test_a_sample_s_new_exposures_depend_on_its_own_row_only(K):
    N = 40
    X, W, H = fr.case_state(K, N, 96, 0)
    full = engine(X, W, H)
    full.kl_step(1, 0)
    Hfull = full.download_H()
    full.close()
    rng = np.random.default_rng(K)
    for n in (17, 16, 1):
        rows = rng.permutation(N)[:n]
        e = engine(X[rows], W, H[rows])
        e.kl_step(1, 0)
        assert np.array_equal(e.download_H(), Hfull[rows]), f"{n} rows of {N}"
        e.close()


# ------------------------------------------------------------------ the shadows follow the state


def _fresh_matches(e, X, g=0, what=""):
    """The next fp32 step of ``e`` equals that of a fresh fp32 engine loaded with ``e``'s state (and ``X``)."""
    W, H = state_of(e)
    ref = engine(X, W, H)
    e.kl_step(1, g), ref.kl_step(1, g)
    ok = same_state(e, ref)
    ref.close()
    assert ok, what


@pytest.mark.parametrize("K", [7, 36])
def test_the_shadow_copies_follow_every_change_of_the_state(K):
    N, V = 39, 83
    X, W, H = fr.case_state(K, N, V, 0)
    rng = np.random.default_rng(K)
    e = engine(X, W, H)
    e.kl_step(2, 0)
    # new counts, through every ingest type: the fp32 copy of X is rebuilt
    Xi = rng.poisson(np.asarray(X) + 0.5)
    for Xnew in (rng.permutation(np.asarray(X)), Xi.astype(np.float32), Xi[::-1].astype(np.int32), (Xi + 1).astype(np.uint16)):
        e.upload_X(Xnew)
        X = np.asarray(Xnew, dtype=np.float64)
        _fresh_matches(e, X, what=f"after upload_X({Xnew.dtype})")
    # new factors
    e.upload_H(rng.permutation(np.asarray(H)))
    _fresh_matches(e, X, what="after upload_H")
    e.upload_W(np.asarray(W)[::-1].copy())
    _fresh_matches(e, X, what="after upload_W")
    # fp64 kernels that rewrite H or W between fp32 steps
    e.update_H()
    _fresh_matches(e, X, what="after update_H")
    e.update_W(0)
    _fresh_matches(e, X, what="after update_W")
    e.set_precision("f64")
    e.kl_step(1, 0)
    e.set_precision("f32")
    _fresh_matches(e, X, what="after an fp64 kl_step")
    # a kept step and its rollback, in either mode
    for precision in ("f32", "f64"):
        before = state_of(e)
        e.set_precision(precision)
        e.kl_step_objective(0, 2, 0, keep=True)
        e.objective_read(0, 1)
        e.kl_rollback()
        e.set_precision("f32")
        assert all(np.array_equal(a, b) for a, b in zip(before, state_of(e))), f"rollback in {precision}"
        _fresh_matches(e, X, what=f"after kl_step_objective(keep) + kl_rollback in {precision}")
    # f32 -> f64 -> f32 with nothing in between
    e.set_precision("f64"), e.set_precision("f32")
    _fresh_matches(e, X, what="after f32 -> f64 -> f32")
    e.close()


# ------------------------------------------------------------------ hand-back hygiene

HYGIENE_K = [3, 7, 12, 19, 36, 49, 60]  # one per KS in {1, 2, 4, 8, 10, 13, 16}; 19, 36, 49 have remainder columns in the fp64 pass
FP64_OPS = {
    "kl_step": lambda e: e.kl_step(2, 0),
    "update_H": lambda e: e.update_H(),
    "update_W": lambda e: e.update_W(0),
    "objective": lambda e: e.objective(),
    "samplewise_kl": lambda e: e.samplewise_kl(),
    "reconstruct": lambda e: e.reconstruct(),
    "mv_step": lambda e: e.mv_step(1, 0, 1.0, 1.0, 1.0),
}


@pytest.mark.parametrize("small_tiles", [0, 64])
@pytest.mark.parametrize("K", HYGIENE_K)
def test_nothing_the_fp32_pass_leaves_in_the_padding_of_h_is_seen_by_an_fp64_kernel(K, small_tiles):
    """Three fp32 steps write filler into the pad rows and columns of the fp32 H, and the hand-back copies all of it over
    the fp64 H.  Every fp64 kernel must then give what it gives on a fresh engine that was uploaded the downloaded W and H
    (pad columns 0, pad rows 1).  ``small_tiles = 64``: the one-workgroup kernel reads that H where K <= 16."""
    N, V = 39, 83
    X, W, H = fr.case_state(K, N, V, 0)
    for name, op in FP64_OPS.items():
        e = engine(X, W, H, small_tiles=small_tiles)
        e.kl_step(3, 0)
        e.set_precision("f64")
        Wd, Hd = state_of(e)
        ref = engine(X, Wd, Hd, precision="f64", small_tiles=small_tiles)
        got, want = op(e), op(ref)
        assert np.array_equal(np.asarray(got), np.asarray(want)), f"{name}: return values differ"
        assert same_state(e, ref), f"{name}: the state differs"
        e.close(), ref.close()


# ------------------------------------------------------------------ a poisoned sample, determinism


def test_a_nan_in_one_sample_spreads_as_in_the_oracle():
    K, N, V = 12, 39, 96
    X, W, H = (np.array(a) for a in fr.case_state(K, N, V, 0))
    X[21, 40] = np.nan
    e = engine(X, W, H)
    e.kl_step(1, 0)
    Wd, Hd = state_of(e)
    e.close()
    with np.errstate(invalid="ignore"):
        Wo, Ho = (a.T for a in orc.update_WH(X.T, W.T, H.T))
    assert np.isnan(Ho[21]).all() and not np.isnan(np.delete(Ho, 21, axis=0)).any()
    for dev, ref in ((Hd, Ho), (Wd, Wo)):
        assert np.array_equal(np.isnan(dev), np.isnan(ref)) and np.array_equal(np.isinf(dev), np.isinf(ref))
    # and the other samples' exposures are the unpoisoned run's, within the bound
    keep = np.arange(N) != 21
    Hn, _, Hp, _ = fr.exact_step(X[keep], W, H[keep], 0)
    _report("poisoned (H of the other samples)", fr.check(Hd[keep], Hn, Hp, fr.bound_H(K, V), "poison/H"), 0.0)


@pytest.mark.parametrize("K,N,V,g", [(8, 39, 83, 2), (53, 39, 96, 0)])
def test_the_same_call_from_the_same_state_gives_the_same_bits(K, N, V, g):
    X, W, H = fr.case_state(K, N, V, g)
    a, b = engine(X, W, H), engine(X, W, H)
    a.kl_step(3, g), b.kl_step(3, g)
    assert same_state(a, b)
    first = state_of(a)
    a.upload_W(W), a.upload_H(H)
    a.kl_step(3, g)
    assert all(np.array_equal(x, y) for x, y in zip(first, state_of(a)))
    a.close(), b.close()
