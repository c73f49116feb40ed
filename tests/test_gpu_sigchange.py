"""``sal.signature_change_test`` on the device: the free fits against the two
``sal.assign_signatures(candidates=C, required=C)`` calls of the contract, the tied solve at a fixed step count against the
replica's longdouble run (tests/_sigchange_ref.py; tolerance 16 x the float64 spread measured on the CPU on these inputs,
tests/test_sigchange_host.py), the tie itself, the identical-rows and swap identities, the draws against the replica from the
device's own tied exposures, the reduction against its stated rules, and the calibration pairs of tests/test_sigchange_host.py.
``np.array_equal`` unless stated."""

import numpy as np
import pytest

import _refit_ref as refit_ref
import _sigchange_ref as ref
import salamander_amd as sal
from salamander_amd import _lib

pytestmark = pytest.mark.gpu

N = ref.GPU_N
B = 3
SEED = 12345678901234567
CASES = ref.GPU_CASES
H_TOL, F_TOL = 16 * ref.H_SPREAD, 16 * ref.F_SPREAD
EPS64 = float(np.finfo(np.float64).eps)
NAMES = ("statistic", "p_value", "n_exceed", "tested", "null_mean", "share_a", "share_b", "share_difference", "tied_share", "exposures_a",
         "exposures_b", "tied_exposures_a", "tied_exposures_b", "errors", "n_iterations", "converged", "null_statistics", "null_n_iterations", "draws")
PER_DRAW = ("null_statistics", "null_n_iterations", "draws")

_results = {}


def run_of(K, V, fit="fixed"):
    """One call per case and iteration rule, shared by the tests that read it (none changes it)."""
    if (K, V, fit) not in _results:
        Xa, Xb, W, C, test = ref.gpu_case(K, V)
        kw = ref.GPU_FIXED if fit == "fixed" else ref.GPU_FIT
        _results[K, V, fit] = (Xa, Xb, W, C, test, sal.signature_change_test(Xa, Xb, W, test, n_draws=B, seed=SEED, candidates=C, keep_draws=True, **kw))
    return _results[K, V, fit]


def same(one, other, names=NAMES):
    for name in names:
        assert np.array_equal(getattr(one, name), getattr(other, name), equal_nan=True), name


@pytest.mark.parametrize("K,V", CASES)
def test_untested_problems_and_shapes(K, V):
    Xa, Xb, W, C, test, res = run_of(K, V)
    S = len(test)
    want = ref.tested_problems(Xa, Xb, C, test)
    ns, js, _ = ref.gpu_problems(K, V)
    assert res.tested.dtype == bool and np.array_equal(res.tested, want) and np.array_equal(res.candidates, C) and res.test == tuple(test)
    assert ns.size % 2 == 1 and ns.size > 8  # several tiles of 8 problems, the last partly filled
    assert not want[[0, 5, 9]].any() and want[1:5].any(axis=1).all() and (~C[:, list(test)] & (C.sum(axis=1) > 1)[:, None]).any()
    for name in ("statistic", "p_value", "null_mean", "share_a", "share_b", "share_difference", "tied_share"):
        assert getattr(res, name).shape == (N, S) and np.array_equal(np.isnan(getattr(res, name)), ~want), name
    for name, width in (("tied_exposures_a", K), ("tied_exposures_b", K), ("errors", 4)):
        got = getattr(res, name)
        assert got.shape == (N, S, width) and np.array_equal(np.isnan(got).all(axis=2), ~want) and not np.isnan(got[want]).any(), name
    for name in ("exposures_a", "exposures_b"):
        got = getattr(res, name)
        assert got.shape == (N, K) and np.array_equal(np.isnan(got).all(axis=1), ~want.any(axis=1)) and not np.isnan(got[want.any(axis=1)]).any(), name
    assert res.null_statistics.shape == (B, N, S) and np.array_equal(np.isnan(res.null_statistics), np.broadcast_to(~want, (B, N, S)))
    assert res.draws.shape == (B, N, S, 2, V) and not res.draws[:, ~want].any()
    assert res.n_iterations.shape == (N, S, 3) and res.null_n_iterations.shape == (B, N, S, 3)
    assert not res.n_exceed[~want].any() and not res.n_iterations[~want].any() and not res.null_n_iterations[:, ~want].any()
    assert res.n_iterations.dtype == np.int32 and res.n_exceed.dtype == np.int32 and res.converged.dtype == bool and not res.converged[~want].any()


@pytest.mark.parametrize("K,V", CASES)
@pytest.mark.parametrize("fit", ["fixed", "rule"])
def test_free_fits_are_the_two_masked_solves(K, V, fit):
    """Under the convergence rule the two sides of a pair stop at different tests, and the earlier one waits."""
    Xa, Xb, W, C, test, res = run_of(K, V, fit)
    kw = ref.GPU_FIXED if fit == "fixed" else ref.GPU_FIT
    rows = np.flatnonzero(res.tested.any(axis=1))
    ns, js, _ = ref.gpu_problems(K, V)
    for side, (X, H) in enumerate(((Xa, res.exposures_a), (Xb, res.exposures_b))):
        free = sal.assign_signatures(X[rows], W, candidates=C[rows], required=C[rows], **kw)
        at = np.searchsorted(rows, ns)  # the row of `free` of every tested problem
        assert np.array_equal(H[rows], free.exposures), side
        assert np.array_equal(res.errors[ns, js, side], free.reconstruction_errors[at]), side
        assert np.array_equal(res.n_iterations[ns, js, side], free.n_iterations[at]) and np.array_equal(res.converged[ns, js, side], free.converged[at]), side
        assert (H[rows][~C[rows]] == 0.0).all()
    e = res.errors[ns, js]
    assert np.array_equal(res.statistic[ns, js], (e[:, 2] - e[:, 0]) + (e[:, 3] - e[:, 1]))
    if fit == "rule" and K < 96:  # (tests/test_sigchange_host.py shows it on the replica's counts: a side waits two tests or more)
        assert (np.abs(res.n_iterations[ns, js, 0] - res.n_iterations[ns, js, 1]) >= 2 * kw["conv_test_freq"]).any()
        assert 1 < np.unique(res.n_iterations[ns, js, 2]).size
    ta, tb = np.maximum(Xa, ref.EPSILON).sum(axis=1), np.maximum(Xb, ref.EPSILON).sum(axis=1)
    sig = np.asarray(test)[js]
    assert np.array_equal(res.share_a[ns, js], res.exposures_a[ns, sig] / ta[ns]) and np.array_equal(res.share_b[ns, js], res.exposures_b[ns, sig] / tb[ns])
    assert np.array_equal(res.share_difference[ns, js], res.share_b[ns, js] - res.share_a[ns, js])


@pytest.mark.parametrize("K,V", CASES)
def test_tied_solve_against_the_longdouble_replica(K, V):
    Xa, Xb, W, C, test, res = run_of(K, V)
    ns, js, sig = ref.gpu_problems(K, V)
    _, _, ld, (scale_a, scale_b) = ref.fixed_spread(K, V)
    got_a, got_b = res.tied_exposures_a[ns, js], res.tied_exposures_b[ns, js]
    dh, df = ref.deviations(got_a, got_b, res.errors[ns, js, 2], res.errors[ns, js, 3], ld, C[ns], scale_a, scale_b)
    print(f"K = {K}, V = {V}: tied exposures within {dh:.3g} (tolerance {H_TOL:.3g}), divergences within {df:.3g} (tolerance {F_TOL:.3g})")
    assert dh <= H_TOL and df <= F_TOL
    assert (got_a[~C[ns]] == 0.0).all() and (got_b[~C[ns]] == 0.0).all()
    assert np.array_equal(res.n_iterations[ns, js, 2], np.full(ns.size, 40))
    # the tie: off the floor both tied entries are tied_share x t, and the two shares agree to the roundings of the steps
    rows = np.arange(ns.size)
    ha, hb = got_a[rows, sig], got_b[rows, sig]
    ta, tb = np.maximum(Xa[ns], ref.EPSILON).sum(axis=1), np.maximum(Xb[ns], ref.EPSILON).sum(axis=1)
    off = (ha > ref.EPSILON) & (hb > ref.EPSILON)
    assert off.sum() >= ns.size // 2
    share = res.tied_share[ns, js]
    assert (np.abs(ha - share * ta)[off] <= H_TOL * ha[off]).all() and (np.abs(hb - share * tb)[off] <= H_TOL * hb[off]).all()
    tie = np.abs(ha / ta - hb / tb)[off] / share[off]
    bound = (ref.TIE_ROUNDINGS_PER_STEP * 40 + 4) * EPS64
    print(f"K = {K}, V = {V}: the two tied shares part by at most {tie.max():.3g} (bound {bound:.3g}), {int(off.sum())} of {ns.size} off the floor")
    assert (tie <= bound).all()


@pytest.mark.parametrize("K,V", CASES[1:])
def test_identical_rows(K, V):
    Xa, Xb, W, C, test, res = run_of(K, V)
    twin = sal.signature_change_test(Xa, Xa, W, test, n_draws=1, candidates=C, **ref.GPU_FIT)
    ns, js = np.nonzero(twin.tested)
    assert ns.size > 8 and (twin.statistic[ns, js] == 0.0).all()
    for side, H in enumerate((twin.tied_exposures_a, twin.tied_exposures_b)):
        assert np.array_equal(H[ns, js], twin.exposures_a[ns]) and np.array_equal(twin.errors[ns, js, 2 + side], twin.errors[ns, js, 0]), side
    assert np.array_equal(twin.n_iterations[ns, js, 2], twin.n_iterations[ns, js, 0]) and np.array_equal(twin.converged[ns, js, 2], twin.converged[ns, js, 0])


def test_equal_shares():
    """b = m a with nothing clipped and nothing at the floor (tests/test_sigchange_host.py): the tied solve is the free solves."""
    Da, Dw = ref.dense_case(N=12)
    for m in (2.0, 4.0):
        scaled = sal.signature_change_test(Da, m * Da, Dw, (0, 3), n_draws=1, **ref.GPU_FIXED)
        assert scaled.tested.all() and (scaled.statistic == 0.0).all()
        for j in range(2):
            assert np.array_equal(scaled.tied_exposures_a[:, j], scaled.exposures_a) and np.array_equal(scaled.tied_exposures_b[:, j], scaled.exposures_b)


@pytest.mark.parametrize("K,V", CASES)
@pytest.mark.parametrize("fit", ["fixed", "rule"])
def test_swapped_sides(K, V, fit):
    """(b, a) gives the same statistic and the sides' results exchanged, bit for bit: at K = 96 the tested signatures sit in
    the first, the third and the last 16-row tile, so an exchange selected by the wrong (kt, r, q) shows here too."""
    Xa, Xb, W, C, test, one = run_of(K, V, fit)
    other = sal.signature_change_test(Xb, Xa, W, test, n_draws=1, seed=SEED, candidates=C, **(ref.GPU_FIXED if fit == "fixed" else ref.GPU_FIT))
    assert one.tested.sum() > 8 and (one.statistic[one.tested] != 0.0).any()
    same(one, other, ("statistic", "tested", "tied_share"))
    for mine, theirs in (("exposures_a", "exposures_b"), ("tied_exposures_a", "tied_exposures_b"), ("share_a", "share_b")):
        assert np.array_equal(getattr(one, mine), getattr(other, theirs), equal_nan=True), mine
        assert np.array_equal(getattr(one, theirs), getattr(other, mine), equal_nan=True), mine
    for name in ("errors", "n_iterations", "converged"):
        assert np.array_equal(getattr(one, name)[..., [1, 0] + ([3, 2] if name == "errors" else [2])], getattr(other, name), equal_nan=True), name


@pytest.mark.parametrize("K,V", CASES)
def test_draws_equal_the_replica(K, V):
    Xa, Xb, W, C, test, res = run_of(K, V)
    want = ref.draws_from(res.tied_exposures_a, res.tied_exposures_b, refit_ref.normalize(W), Xa.sum(axis=1), Xb.sum(axis=1), test, res.tested, B, SEED)
    assert np.array_equal(res.draws, want)
    totals = np.where(res.tested[:, :, None], np.stack([Xa.sum(axis=1), Xb.sum(axis=1)], axis=1)[:, None, :], 0.0)
    assert np.array_equal(res.draws.sum(axis=4), np.broadcast_to(totals, (B, N, len(test), 2)))
    n, j = 3, int(np.flatnonzero(res.tested[3])[0])
    assert V == 1 or not np.array_equal(res.draws[0, n, j, 1], res.draws[1, n, j, 1])  # (with one feature every draw is the row's total)


@pytest.mark.parametrize("K,V", CASES)
def test_null_statistics_are_the_procedure_on_the_kept_draws(K, V):
    Xa, Xb, W, C, test, res = run_of(K, V)
    ns, js, sig = ref.gpu_problems(K, V)
    worst = 0.0
    for b in range(B):
        da, db = res.draws[b, ns, js, 0], res.draws[b, ns, js, 1]
        a = sal.assign_signatures(da, W, candidates=C[ns], required=C[ns], **ref.GPU_FIXED)
        bb = sal.assign_signatures(db, W, candidates=C[ns], required=C[ns], **ref.GPU_FIXED)
        ld = ref.tied_solve(da, db, W, C[ns], sig, dtype=np.longdouble, **ref.GPU_FIXED)
        assert np.array_equal(res.null_n_iterations[b, ns, js], np.stack([a.n_iterations, bb.n_iterations, ld.n_iterations], axis=1)), b
        want = ((ld.errors_a - a.reconstruction_errors) + (ld.errors_b - bb.reconstruction_errors)).astype(np.float64)
        scale_a, scale_b = ref.row_scales(da, db, W, ld.exposures_a, ld.exposures_b)
        worst = max(worst, float((np.abs(res.null_statistics[b, ns, js] - want) / ((F_TOL + 4 * EPS64) * (scale_a + scale_b))).max()))
    print(f"K = {K}, V = {V}: null statistics at {worst:.3g} of their tolerance")
    assert worst <= 1.0


@pytest.mark.parametrize("K,V", CASES)
def test_reduction(K, V):
    *_, res = run_of(K, V)
    n_exceed, mean, p = ref.reduce_null(res.statistic, res.null_statistics)
    assert np.array_equal(res.n_exceed, n_exceed) and np.array_equal(res.null_mean, mean, equal_nan=True) and np.array_equal(res.p_value, p, equal_nan=True)
    with np.errstate(invalid="ignore"):
        assert np.array_equal(res.n_exceed, (res.null_statistics >= res.statistic).sum(axis=0))
    assert np.array_equal(res.p_value[res.tested], (1 + res.n_exceed[res.tested]) / (B + 1))
    for key in ("draw_s", "solve_s", "reduce_s", "total_s", "sigchange_kernel_ms"):
        assert res.timings[key] >= 0.0
    assert res.timings["n_chunks"] == 1


def test_a_problem_does_not_depend_on_the_draws_the_other_pairs_or_the_other_signatures():
    Xa, Xb, W, _, test = ref.gpu_case(17, 96)
    kw = dict(seed=3, keep_draws=True, **ref.GPU_FIT)
    eight = sal.signature_change_test(Xa, Xb, W, test, n_draws=8, **kw)
    four = sal.signature_change_test(Xa, Xb, W, test, n_draws=4, **kw)
    assert eight.candidates is None and np.array_equal(eight.tested, ref.tested_problems(Xa, Xb, np.ones((N, 17), dtype=bool), test))
    same(four, eight, [name for name in NAMES if name not in PER_DRAW + ("p_value", "n_exceed", "null_mean")])
    for name in PER_DRAW:
        assert np.array_equal(getattr(four, name), getattr(eight, name)[:4], equal_nan=True), name  # B = 4 against the first 4 of B = 8
    # a row subset against the full call: the fits do not see n; the draws do, so the rows that keep their index keep everything
    head = sal.signature_change_test(Xa[:20], Xb[:20], W, test, n_draws=4, **kw)
    for name in NAMES:
        full = getattr(four, name)
        assert np.array_equal(getattr(head, name), full[:, :20] if name in PER_DRAW else full[:20], equal_nan=True), name
    # a subset of the tested signatures: a problem's stream word carries s, not its place in `test`
    one = sal.signature_change_test(Xa, Xb, W, test[1:2], n_draws=4, **kw)
    for name in NAMES:
        full = getattr(four, name)
        if name in ("exposures_a", "exposures_b"):
            assert np.array_equal(getattr(one, name), full, equal_nan=True), name
        else:
            assert np.array_equal(getattr(one, name), full[:, :, 1:2] if name in PER_DRAW else full[:, 1:2], equal_nan=True), name
    assert not np.array_equal(sal.signature_change_test(Xa, Xb, W, test, n_draws=1, seed=4, keep_draws=True, **ref.GPU_FIT).draws[0], four.draws[0])


def test_chunks_give_the_same_bits():
    Xa, Xb, W, C, test, whole = run_of(3, 7)
    problems = int(whole.tested.sum())
    for per_chunk, n_chunks in ((1, 3), (2, 2)):
        res = sal.signature_change_test(Xa, Xb, W, test, n_draws=B, seed=SEED, candidates=C, keep_draws=True, chunk_bytes=per_chunk * problems * 2 * 7 * 8,
                                        **ref.GPU_FIXED)
        assert res.timings["n_chunks"] == n_chunks
        same(res, whole)
    assert sal.signature_change_test(Xa, Xb, W, test, n_draws=2, **ref.GPU_FIXED).draws is None


def test_changed_share_and_calibration():
    """The 64 + 8 pairs of tests/test_sigchange_host.py at the defaults' convergence rule, under the same two conditions (the
    device's solves stop on their own tests, the replica's at a fixed step count: bounds, not equalities).  The device gives 2 of
    64 at or below 0.05 (mean p 0.502), all 8 planted pairs at n_exceed 0, their statistics 16.7 to 24.6 times the largest null one."""
    Xa, Xb, S = ref.calibration_pairs()
    res = sal.signature_change_test(Xa, Xb, S, (ref.CALIBRATION_TEST, 4), n_draws=39, seed=0)
    null = res.p_value[:64, 0]
    ratio = res.statistic[64:, 1] / res.null_statistics[:, 64:, 1].max(axis=0)
    print(f"null pairs: {int((null <= 0.05).sum())} of 64 at or below 0.05, mean p {null.mean():.3f}; planted n_exceed {res.n_exceed[64:, 1]}, "
          f"statistic / largest null {ratio.min():.1f} .. {ratio.max():.1f}; iterations {res.n_iterations.min()}..{res.n_iterations.max()}, "
          f"null {res.null_n_iterations.min()}..{res.null_n_iterations.max()}; smallest statistic {res.statistic.min():.3g}")
    assert res.tested.all()
    assert (null <= 0.05).sum() <= 8
    assert np.array_equal(res.n_exceed[64:, 1], np.zeros(8, dtype=np.int32))


def test_errors_through_the_c_abi():
    lib = _lib.load_with_device()
    p = _lib.pointer
    X = np.ones((4, 10))
    out = dict(tested=np.empty((4, 2), dtype=np.uint8), stat=np.empty((4, 2)), exceed=np.empty((4, 2), dtype=np.int32), mean=np.empty((4, 2)),
               Ha=np.empty((4, 97)), Hb=np.empty((4, 97)), Ha0=np.empty((4, 2, 97)), Hb0=np.empty((4, 2, 97)), err=np.empty((4, 2, 4)),
               nit=np.empty((4, 2, 3), dtype=np.int32), conv=np.empty((4, 2, 3), dtype=np.int32), stat_b=np.empty((5, 4, 2)),
               nit_b=np.empty((5, 4, 2, 3), dtype=np.int32))

    def call(W, n_draws, Xa=X, Xb=X, max_it=20, test=(0, 2)):
        T = np.asarray(test, dtype=np.int32)
        return lib.salnmf_signature_change(0, p(Xa), Xa.shape[0], Xa.shape[1], p(Xb), Xb.shape[0], Xb.shape[1], p(W), W.shape[0], p(T), T.size, None,
                                           n_draws, 0, 10, max_it, 10, 1e-7, 0, *(p(a) for a in out.values()), None, None)

    W = np.full((3, 10), 0.1)
    half = np.where(np.arange(40).reshape(4, 10) == 12, 0.5, X)
    assert call(np.full((97, 10), 0.1), 5) == 1 and "n_signatures must be in [1, 96], got 97" in _lib.last_error()
    assert call(W, 0) == 1 and "n_draws must be in [1, 65536], got 0" in _lib.last_error()
    assert call(W, 5, Xb=np.ones((3, 10))) == 1 and "the shapes must agree, got 4 x 10 and 3 x 10" in _lib.last_error()
    assert call(W, 5, Xa=half) == 1 and "integer counts below 2^32: row 1, column 2 holds 0.5" in _lib.last_error()
    assert call(W, 5, Xb=half) == 1 and "integer counts below 2^32: row 1, column 2 holds 0.5" in _lib.last_error()
    assert call(W, 5, max_it=25) == 1 and "max_iterations must be a multiple of conv_test_freq, got 25 and 10" in _lib.last_error()
    assert call(W, 5, test=(0, 3)) == 1 and "tested signature 3 is not in [0, 3)" in _lib.last_error()
    assert call(W, 5, test=(1, 1)) == 1 and "signature 1 is tested twice" in _lib.last_error()
    assert call(W, 5) == 0 and out["tested"].all() and np.isfinite(out["stat"]).all() and np.isfinite(out["stat_b"]).all()
