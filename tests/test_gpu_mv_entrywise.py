"""The MvNMF W step on the device, entry by entry against an extended-precision reference (``tests/_mv_ref.py``).

The float64 oracle cannot pin these kernels: where ``b = r - 4 lam A > 0`` the closed-form root cancels and the oracle's
own entries are good to ``eps kappa`` only (1e-9 .. 1e-5 on ordinary problems, DESIGN.md "Accuracy of the MvNMF W step").
Here every entry of a device result is compared with the exact value, within a bound that follows the entry's own
conditioning, in three regimes that each isolate one part of the kernel chain:

(a) lam-dominated, b < 0 everywhere: nothing cancels, kappa = 1, Wu is a well-conditioned function of A and B.  Bound
    ``C_a eps cond2(S)`` (< 1e-14): pins the Gram tiles, the elimination at every size class, the on-the-fly
    ``fmax(0, -y)`` / ``fabs(y)`` operands and the k-step remainder of the A / B products.
(b) count-dominated, b > 0 (lam = 1 and 1e-3, counts x 1000): bound ``C_b eps kappa``.  Pins ``mv_root_entry``, the row
    sums of H and the numerator G; r enters amplified by kappa, so a row sum off in its last bits shows here.
(c) ill-conditioned S (delta = 1e-6, 1e-10 with two near or exact duplicate signatures, cond2(S) = 1e5, 1e9): the only
    place where the elimination without pivoting meets pivots that span nine orders.  Bound ``C_c eps cond2(S)``.

``C`` is 4 x the largest ratio the float64 oracle itself reaches in the regime (``_mv_ref.C``, measured and asserted in
``test_mv_ref_host.py``): not tuned on the device.  Every assertion names the failing (k, v), its kappa and its ratio.
The measured device ratios are printed (run with ``-s``) and recorded in DESIGN.md.
"""

import ctypes
import functools
import os
import sys

import mpmath as mp
import numpy as np
import pytest

import _mv_ref as R
from oracle import klnmf_oracle as orc
from salamander_amd import _lib
from salamander_amd.engine import Engine

pytestmark = pytest.mark.gpu

EPS = R.EPS64


@functools.lru_cache(maxsize=None)
def _case(V, N, K, delta, scale=1.0, duplicates=None):
    """(X, W, H, MvRef): the mpmath work of a case is done once per module run"""
    X, W, H = R.problem(V, N, K, scale, duplicates)
    return X, W, H, R.MvRef(W, delta, X, H)


@pytest.fixture(scope="module", autouse=True)
def _release_cases():
    yield
    _case.cache_clear()  # (mpf object arrays and 20 000-sample matrices: not kept for the rest of the session)


def _read_reduction(e, K, V):
    """``[G (K, V) | rowsums_H (K)]`` as the last W step left them on the device (``SALNMF_BUF_RED``)."""
    hip = ctypes.CDLL(_lib.mapped_runtime_libraries()["libamdhip64"][0])
    out = np.empty(K * V + K + 1)
    e.sync()
    rc = hip.hipMemcpy(ctypes.c_void_p(out.ctypes.data), ctypes.c_void_p(e.device_ptr(_lib.BUF_RED)), ctypes.c_size_t(out.nbytes), 2)
    assert rc == 0, rc
    return out[: K * V].reshape(K, V).copy(), out[K * V : K * V + K].copy()


def _engine(X, W, H):
    e = Engine(X.shape[0], X.shape[1], W.shape[0])
    e.upload_X(X), e.upload_W(W), e.upload_H(H)
    return e


def _check(tag, got, u, ref, regime, want_b_neg=None, c_neg=None):
    """Every entry of ``got`` within ``_mv_ref.bound``; given rows and clipped entries exactly.  Returns the worst ratio
    (error / (eps * unit), unit = kappa where b > 0 and cond2(S) elsewhere) for the record."""
    assert np.isfinite(got).all(), tag
    assert np.array_equal(got[u.given], ref.W[u.given]), f"{tag}: given rows changed"
    live = ~u.given & ~u.ambiguous
    assert u.ambiguous.mean() <= 1e-3 and (regime == "b" or not u.ambiguous.any()), tag
    assert np.array_equal(got[live & u.clipped], np.full((live & u.clipped).sum(), R.EPSILON)), f"{tag}: clipped entries differ from EPSILON"
    if want_b_neg is not None:
        assert abs((u.b < 0).mean() - want_b_neg) <= 0.005, (tag, (u.b < 0).mean())
    err = np.where(live, u.rel_err(got), 0.0)
    allowed = R.bound(u, ref, regime, c_neg)
    over = err / allowed
    k, v = np.unravel_index(np.argmax(over), over.shape)
    unit = np.where(u.b > 0, u.kappa, ref.cond)
    ratio = float((err / (EPS * unit)).max())
    print(f"\n[mv-entrywise] {tag} regime {regime}: worst error / (eps x unit) {ratio:.3f} (unit: kappa where b > 0, cond2(S) elsewhere), "
          f"worst entry at {over[k, v]:.3f} of its bound, max rel err {err.max():.2e}, cond {ref.cond:.3g}, kappa max {u.kappa.max():.2g}")
    assert over[k, v] <= 1.0, (
        f"{tag}: entry (k={k}, v={v}) off by {err[k, v]:.3e} relative = {over[k, v]:.2f} x its bound {allowed[k, v]:.3e}; "
        f"kappa {u.kappa[k, v]:.3e}, b {u.b[k, v]:.3e}, cond2(S) {ref.cond:.3e}, exact {float(u.Wu[k, v]):.17g}, got {got[k, v]:.17g}; "
        f"{int((over > 1).sum())} entries over")
    return ratio


def _check_logdet(tag, e, ref):
    got = e.mv_logdet(ref.delta)
    err = abs(float(mp.mpf(got) - ref.logdet))
    allowed = R.C["logdet"] * EPS * ref.logdet_scale
    print(f"\n[mv-entrywise] {tag} logdet: ratio {err / (EPS * ref.logdet_scale):.3f} (x eps x {ref.logdet_scale:.3g}), allowed {R.C['logdet']:.2f}")
    assert err <= allowed, f"{tag}: log det {got!r} vs {float(ref.logdet)!r}: off by {err:.3e}, allowed {allowed:.3e}"


# K: every size class of the elimination's work split (test_mvnmf_w_only_algebra_every_size); V: full, ragged, tiny -- the
# row clamps min(.., K - 1) and the masks m < K of the Gram / A-B loops hit both remainders at K = 17, 33, 57 with V = 7, 83
# (K, V, n_given, N); N = 900 + K is ragged; the last one has a cooperative leftover tile (regimes (a) and (b) both)
LDS_CASES = [(2, 96, 1, 902), (3, 83, 2, 903), (5, 7, 0, 905), (8, 96, 7, 908), (16, 83, 0, 916), (17, 7, 0, 917), (22, 96, 2, 922),
             (23, 83, 2, 923), (31, 7, 30, 931), (33, 83, 32, 933), (42, 96, 0, 942), (43, 7, 42, 943), (45, 83, 44, 945),
             (50, 96, 49, 950), (57, 7, 2, 957), (64, 83, 0, 964), (17, 83, 2, 917), (33, 7, 2, 933), (57, 83, 56, 957),
             (64, 96, 2, 964), (30, 96, 0, 17003)]
# feature blocks (V > 96), signature chunks with the K x K algebra in global memory (K > 64), both
SPLIT_CASES = [(8, 288, 7, 908), (12, 250, 2, 912), (65, 96, 64, 965), (100, 83, 0, 1000), (130, 96, 2, 1030), (100, 288, 2, 1000)]


@pytest.mark.parametrize("K,V,n_given,N", LDS_CASES + SPLIT_CASES)
def test_unconstrained_update_and_logdet_entry_by_entry(K, V, n_given, N):
    """``mv_update_W_unconstrained`` (the stand-alone 1024-thread algebra, or its feature-block / signature-chunk forms) and
    ``mv_logdet`` from an uploaded state, ragged N, in regimes (a) and (b) (lam = 1 and lam = 1e-3), with 0, 2 or K - 1
    given signatures."""
    delta = 1.0
    X, W, H, ref = _case(V, N, K, delta)
    e = _engine(X, W, H)
    tag = f"K={K} V={V} N={N} given={n_given}"
    _check_logdet(tag, e, ref)
    lam_a = R.lam_dominated(ref)
    u = ref.update_W_unconstrained(lam_a, n_given)
    _check(f"{tag} lam={lam_a:.3g}", e.mv_update_W_unconstrained(n_given, lam_a, delta), u, ref, "a", want_b_neg=0.99 if K == 2 else 1.0)  # (share measured on the CPU; b >= 0 entries are bounded as in (b))
    for lam in (1.0, 1e-3):
        u = ref.update_W_unconstrained(lam, n_given)
        assert (u.b > 0).all()
        got = e.mv_update_W_unconstrained(n_given, lam, delta)
        _check(f"{tag} lam={lam}", got, u, ref, "b")
        if K <= 64 and V <= 96:
            _check_restated(f"{tag} lam={lam}", e, got, u, ref, lam, n_given)
    e.close()


def _check_restated(tag, e, got, u, ref, lam, n_given):
    """The device's root against the reference's statements in float64, operation for operation
    (``_mv_ref.restated_root``), from the device's own G and row sums (read back) and the exact A, B rounded to float64.

    Where b > 0, the device's A differs from the exact one by ``C_a eps cond2(S)`` relative, i.e. by < 1e-4 ulp of
    ``b = r - 4 lam A`` (4 lam A is 1e5 .. 1e9 times smaller than r), and its B moves ``b^2 + 8 lam B G`` by ~1 / kappa ulp:
    b and the root come out bit for bit the same except on a share of entries of the order 40 / kappa + 1e-4, and B's own
    error then passes to Wu through the final division alone, not amplified.  So all but 1 % of the entries agree to
    ``(C_a cond2(S) + 4) eps`` (the others are still held by the eps kappa bound of ``_check``) -- four to ten orders
    below eps kappa.  A multiply-add contracted into the root skips the rounding of ``b^2`` and moves about every second
    entry by ~kappa eps / 4."""
    G, r = _read_reduction(e, ref.K, ref.V)
    want = R.restated_root(ref.W, R.to_float(ref.A), R.to_float(ref.B), G, r, lam, n_given)
    live = ~u.given & ~u.clipped & ~u.ambiguous
    err = np.where(live, np.abs(got - want) / want, 0.0)
    tol = (R.C["a"] * ref.cond + 4) * EPS
    share = float((err[live] > tol).mean())  # (of the live entries: given rows agree trivially)
    print(f"\n[mv-entrywise] {tag} restated root: {share:.4f} of the entries beyond {tol / EPS:.0f} eps, median {np.median(err[live]) / EPS:.2f} eps, "
          f"max {err.max() / EPS:.3g} eps (kappa min {u.kappa[live].min():.2g})")
    k, v = np.unravel_index(np.argmax(err), err.shape)
    assert share <= 0.01, (f"{tag}: {share:.3f} of the entries differ from the float64 restatement of the root by more than {tol:.2e}; "
                           f"worst (k={k}, v={v}): {err[k, v]:.3e} at kappa {u.kappa[k, v]:.3e}")


@pytest.mark.parametrize("V,N,K,lam,delta,scale", [(96, 900, 8, 0.7, 0.3, 1.0), (96, 3000, 12, 1.0, 1.0, 1.0), (96, 20000, 30, 1.0, 1.0, 1.0),
                                                   (96, 20000, 30, 1e-3, 1.0, 1.0), (96, 3000, 12, 1.0, 1.0, 1000.0), (83, 17003, 33, 1.0, 1.0, 1.0)])
def test_count_dominated_cases_of_the_accuracy_table(V, N, K, lam, delta, scale):
    """Regime (b) on the five cases of the table in DESIGN.md (the oracle reaches 0.55 .. 0.90 eps kappa there) and one
    with a cooperative leftover tile and ragged V: r and G over many tiles and workgroup slabs feed the root."""
    X, W, H, ref = _case(V, N, K, delta, scale)
    e = _engine(X, W, H)
    u = ref.update_W_unconstrained(lam)
    assert (u.b > 0).all() and not u.clipped.any()
    _check(f"V={V} N={N} K={K} lam={lam} delta={delta} counts x{scale:g}", e.mv_update_W_unconstrained(0, lam, delta), u, ref, "b")
    e.close()


@pytest.mark.parametrize("delta,duplicates,lam_factor", [(1e-6, "near", 25.0), (1e-10, "near", 25e5), (1e-6, "exact", 25.0), (1e-10, "exact", 25e5)])
def test_ill_conditioned_gram_matrix(delta, duplicates, lam_factor):
    """Regime (c): pivots over five and nine orders of magnitude in the elimination without pivoting; with exact
    duplicates S is semi-definite but for delta.  Finite results within ``C_c eps cond2(S)``, log det within the pivot
    bound; with the lam rule of regime (a) unchanged at delta = 1e-10, half the entries have b > 0 and are bounded by the
    first-order sum of both effects (``_mv_ref.bound``)."""
    X, W, H, ref = _case(96, 900, 8, delta, 1.0, duplicates)
    e = _engine(X, W, H)
    tag = f"delta={delta} {duplicates} duplicates"
    _check_logdet(tag, e, ref)
    lam = R.lam_dominated(ref, lam_factor)
    _check(f"{tag} lam={lam:.3g}", e.mv_update_W_unconstrained(0, lam, delta), ref.update_W_unconstrained(lam), ref, "c", want_b_neg=1.0,
           c_neg=R.SLACK * R.ORACLE_RATIO_C[(delta, duplicates)])
    if delta == 1e-10:
        lam = R.lam_dominated(ref)
        _check(f"{tag} lam={lam:.3g}", e.mv_update_W_unconstrained(0, lam, delta), ref.update_W_unconstrained(lam), ref, "c", want_b_neg=0.5,
               c_neg=R.SLACK * R.ORACLE_RATIO["c"])  # (b < 0 entries of this lam: no per-case measurement, the regime's constant)
    e.close()


def test_entries_below_the_floor_are_clipped_to_epsilon_exactly():
    X, W, H = R.clip_problem()
    ref = R.MvRef(W, 1.0, X, H)
    u = ref.update_W_unconstrained(1.0)
    assert u.clipped.sum() >= 3 and not u.ambiguous.any()
    e = _engine(X, W, H)
    got = e.mv_update_W_unconstrained(0, 1.0, 1.0)
    assert np.array_equal(got == R.EPSILON, u.clipped)
    _check("clip case", got, u, ref, "b")
    e.close()


@pytest.mark.parametrize("queued", [True, False])
@pytest.mark.parametrize("K,V", [(8, 96), (17, 7), (23, 83), (33, 83), (43, 7), (57, 83), (64, 96)])
def test_second_step_of_one_call_runs_the_algebra_in_the_spare_workgroup(K, V, queued):
    """Steps 2.. of one ``mv_step`` call evaluate the K x K algebra in the 256-thread spare workgroup of the update_H pass
    (runs of 1, 2, 4, 8 and 16 columns per thread at K = 8, 17, 23, 33 and 43 .. 64; the 16-column form has no other user).
    The state after ``mv_step(2)`` against the exact step 2 started from the device's own state after step 1 -- one step's
    error, not two steps' propagated -- in regime (a), queued and classic forms, plus bit-equality with two single-step
    calls.  Also here: the state after the single ``mv_step(1)`` call against the exact step 1, and ``mv_update_W`` (the
    stand-alone W update from an uploaded state) against the same.

    Bound per entry of W: ``eps (C_a cond2(S) + 8 + 2 sqrt(K + V))``.  ``8``: normalising the accepted trial (a V-term sum
    of positive numbers in a two-level order, one division, as in the line-search test).  The last term only where the
    device ran ``update_H`` itself: whichever precision the reference's H has, the device's entries carry the roundings of
    a K-term and a V-term dot product of positive numbers, ~sqrt(K + V) eps each and independent from sample to sample
    (the worst case, (K + V + 3) eps on every sample with one sign, cannot be met by 900 samples at once); r and G are sums
    over the samples and pass that on with a sensitivity below one in this regime.  ``mv_update_W`` starts from an
    uploaded H and gets no such term."""
    N, delta = 900 + K, 1.0
    X, W, H, ref0 = _case(V, N, K, delta)
    lam = R.lam_dominated(ref0)
    H0 = orc.synthetic_problem(V, N, K, seed=V + N + K)[2]
    one, two, single = _engine(X, W, H0), _engine(X, W, H0), _engine(X, W, H0)
    for e in (one, two, single):
        e.set_mv_queued(queued)
    g1 = one.mv_step(1, 0, lam, delta, 1.0)
    g2 = two.mv_step(2, 0, lam, delta, 1.0)
    gs = single.mv_step(1, 0, lam, delta, single.mv_step(1, 0, lam, delta, 1.0))
    assert g1 == 1.0 and g2 == 1.0 and gs == 1.0  # first trials accepted: the accepted W is the normalised Wu
    upd = _engine(X, W, H)
    upd.set_mv_queued(queued)
    assert upd.mv_update_W(0, lam, delta, 1.0) == 1.0
    W1, H1 = one.download_W(), one.download_H()
    u0 = ref0.update_W_unconstrained(lam)
    want1, _ = ref0.line_search_trial(u0.Wu, H)
    for name, got, extra in (("mv_update_W", upd.download_W(), 0.0), ("step 1", W1, 2 * np.sqrt(K + V))):
        err = R.to_float(abs(R.to_mp(got) - want1) / want1)
        allowed = EPS * (R.C["a"] * ref0.cond + 8 + extra)
        k, v = np.unravel_index(np.argmax(err), err.shape)
        print(f"\n[mv-entrywise] {name} K={K} V={V} queued={queued}: max rel err {err.max() / EPS:.1f} eps, allowed {allowed / EPS:.0f} eps")
        assert err[k, v] <= allowed, f"{name} K={K} V={V} queued={queued}: entry (k={k}, v={v}) off by {err[k, v]:.3e}, allowed {allowed:.3e}"
    upd.close()
    W2 = two.download_W()
    assert np.array_equal(W2, single.download_W()) and np.array_equal(two.download_H(), single.download_H())
    H2 = np.ascontiguousarray(orc.update_H(X.T, W1.T, H1.T).T)
    ref = R.MvRef(W1, delta, X, H2)
    u = ref.update_W_unconstrained(lam)
    assert (u.b < 0).all() and not u.clipped.any()
    want, _ = ref.line_search_trial(u.Wu, H2)
    err = R.to_float(abs(R.to_mp(W2) - want) / want)
    allowed = EPS * (R.C["a"] * ref.cond + 8 + 2 * np.sqrt(K + V))
    k, v = np.unravel_index(np.argmax(err), err.shape)
    print(f"\n[mv-entrywise] step 2 K={K} V={V} queued={queued}: max rel err {err.max():.2e} = {err.max() / EPS:.1f} eps, allowed {allowed / EPS:.0f} eps")
    assert err[k, v] <= allowed, f"K={K} V={V} queued={queued}: entry (k={k}, v={v}) off by {err[k, v]:.3e}, allowed {allowed:.3e} (cond {ref.cond:.3g})"
    for e in (one, two, single):
        e.close()


@pytest.mark.parametrize("V,N,K,lam,delta,gamma_in", [(96, 908, 8, 1.0, 1.0, 1.0), (83, 933, 33, 0.7, 0.3, 0.37), (96, 964, 64, 1.0, 1.0, 1.0)])
def test_line_search_from_the_exact_update(V, N, K, lam, delta, gamma_in):
    """``mv_line_search`` with the exact Wu (rounded to float64) uploaded: the accepted W is normalise + clip only, so every
    entry agrees with the exact trial to ``8 eps`` (the rounding of Wu itself, a V-term sum of positive numbers, one
    division), the rescaled H to the same, gamma exactly (``min(1, 1.2 gamma)``, also from an incoming 0.37: the first trial
    is Wu itself whatever gamma is, ``mvnmf.py:80``; the decision is taken from the reference's own trial); the accepted objective through ``mv_objective`` against
    ``KL + lam log det`` with the KL part in long double (rtol 1e-10 as for the other objective paths) and the log det
    within its pivot bound."""
    X, W, H, ref = _case(V, N, K, delta)
    u = ref.update_W_unconstrained(lam)
    Wu = R.to_float(u.Wu)
    want_W, s = ref.line_search_trial(R.to_mp(Wu), H)
    e = _engine(X, W, H)
    f_prev = e.mv_objective(lam, delta)
    gamma = e.mv_line_search(lam, delta, gamma_in, Wu)
    got_W, got_H = e.download_W(), e.download_H()
    f_new = e.mv_objective(lam, delta)
    # the reference's decision from extended-precision values: the first trial must be better by far more than the error
    L = np.longdouble

    def kl(Wq, Hq):
        P = Hq.astype(L) @ Wq.astype(L)
        Xl = X.astype(L)
        return (Xl * np.log(Xl / P) - Xl + P).sum()

    ref_new = R.MvRef(got_W, delta)
    f0 = float(kl(W, H)) + lam * float(ref.logdet)
    f1 = float(kl(got_W, got_H)) + lam * float(ref_new.logdet)
    want_H = np.maximum(R.to_float(R.to_mp(H) * s[None, :]), R.EPSILON)
    f1_ref = float(kl(R.to_float(want_W), want_H)) + lam * float(R.MvRef(R.to_float(want_W), delta).logdet)
    assert f0 - f1_ref > 1e-6 * abs(f0), "the case must accept its first trial by a margin far above rounding"
    assert gamma == min(1.0, 1.2 * gamma_in)
    err_W = R.to_float(abs(R.to_mp(got_W) - want_W) / want_W)
    err_H = np.abs(got_H - want_H) / want_H
    print(f"\n[mv-entrywise] line search V={V} K={K}: W max {err_W.max() / EPS:.2f} eps, H max {err_H.max() / EPS:.2f} eps, "
          f"objective rel {abs(f_new - f1) / abs(f1):.2e}")
    k, v = np.unravel_index(np.argmax(err_W), err_W.shape)
    assert err_W[k, v] <= 8 * EPS, f"W entry (k={k}, v={v}) off by {err_W[k, v] / EPS:.2f} eps"
    assert err_H.max() <= 8 * EPS, f"H off by {err_H.max() / EPS:.2f} eps"
    kl1 = float(kl(got_W, got_H))
    assert abs(f_new - f1) <= 1e-10 * abs(kl1) + lam * R.C["logdet"] * EPS * ref_new.logdet_scale, (f_new, f1)
    assert abs(f_prev - f0) <= 1e-10 * abs(float(kl(W, H))) + lam * R.C["logdet"] * EPS * ref.logdet_scale, (f_prev, f0)
    e.close()


# ------------------------------------------------------------------ two sample shards: r and G cross the ranks before the root
SHARD_CASE = (96, 3000, 12, 1.0)  # V, N, K, delta: the second row of the accuracy table


def _shard_worker(rank, world, port, out_dir, lams):
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    sys.path.insert(0, root)
    sys.path.insert(0, os.path.join(root, "tests"))
    import torch.distributed as dist

    from salamander_amd.distributed import attach_peer_exchange, shard_bounds

    os.environ["MASTER_ADDR"], os.environ["MASTER_PORT"] = "127.0.0.1", str(port)
    dist.init_process_group("gloo", rank=rank, world_size=world)
    try:
        V, N, K, delta = SHARD_CASE
        X, W, H = R.problem(V, N, K)
        a, b = shard_bounds(N, world, rank)
        e = _engine(X[a:b], W, H[a:b])
        attach_peer_exchange(e)
        assert e.comm_info() == (world, rank, N)
        out = {f"Wu{i}": e.mv_update_W_unconstrained(0, lam, delta) for i, lam in enumerate(lams)}
        out["logdet"] = e.mv_logdet(delta)
        np.savez(os.path.join(out_dir, f"rank{rank}.npz"), **out)
        dist.barrier()  # nobody frees its inbox while a peer may still be inside an exchange
        e.close()
    finally:
        dist.destroy_process_group()


def test_two_sample_shards_on_one_gpu(tmp_path):
    """A 2-rank sample-sharded engine (two processes on one GPU over the peer exchange, the harness of
    ``test_gpu_p2p.py``): the row sums of H and G are all-reduced before the root.  Regime (a) and regime (b) (where a row
    sum off in its last bits is amplified by kappa ~ 1e8), every rank within the bounds of the unsharded engine, and the
    ranks equal bit for bit."""
    import torch.multiprocessing as tmp

    from test_distributed_gloo import _free_port

    V, N, K, delta = SHARD_CASE
    X, W, H, ref = _case(V, N, K, delta)
    lams = [R.lam_dominated(ref), 1.0]
    tmp.spawn(_shard_worker, args=(2, _free_port(), str(tmp_path), lams), nprocs=2, join=True)
    parts = [np.load(os.path.join(tmp_path, f"rank{r}.npz")) for r in range(2)]
    for i, (lam, regime) in enumerate(zip(lams, "ab")):
        u = ref.update_W_unconstrained(lam)
        assert ((u.b < 0) if regime == "a" else (u.b > 0)).all()
        assert np.array_equal(parts[0][f"Wu{i}"], parts[1][f"Wu{i}"])
        for r in range(2):
            _check(f"2 shards, rank {r}, lam={lam:.3g}", parts[r][f"Wu{i}"], u, ref, regime)
    assert float(parts[0]["logdet"]) == float(parts[1]["logdet"])
    assert abs(float(mp.mpf(float(parts[0]["logdet"])) - ref.logdet)) <= R.C["logdet"] * EPS * ref.logdet_scale
