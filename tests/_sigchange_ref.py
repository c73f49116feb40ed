"""A NumPy replica of ``sal.signature_change_test`` (``csrc/salnmf_sigchange.h``) -- TESTS ONLY.

Written from the contract, on ``_presence_ref`` (the solve on a set, the draw under a stream word), ``_gof_ref`` (the reduction),
``_assign_masks_ref`` (the update factors) and ``_change_ref`` (the device test's inputs).  For pair n with clipped rows x_a, x_b,
candidate set C, |C| >= 2, tested signature s in C and both integer totals positive:
    solves a and b: ``_presence_ref.solve`` of x_a and of x_b on C -> (h_a, f_a), (h_b, f_b);
    t the rows' sums, c_a = t_a / (t_a + t_b), c_b = t_b / (t_a + t_b);
    the tied solve: both rows from h_k = t_side / |C| on C; a step multiplies every entry by its own row's update factor, entry s
    of both rows by F = c_a u_as + c_b u_bs, evaluated as (u_as + u_bs) / 2 + ((c_a - c_b) / 2) (u_as - u_bs) with every operation
    rounded, and clips at EPSILON; the objective f_a0 + f_b0 at iteration 0 and at every multiple of conv_test_freq under the
    refit's stop rule, both rows stopping together -> (h_a0, f_a0), (h_b0, f_b0);
    statistic = (f_a0 - f_a) + (f_b0 - f_b);
    null draw b: side a from h_a0 with T_a trials, side b from h_b0 with T_b, under the Philox counter
    (q, 0x53430000 + 2 s + side, n, b); every draw pair goes through the same three solves; the reduction is ``_gof_ref.reduce_null``.
"""

import functools
from types import SimpleNamespace

import numpy as np

import _assign_masks_ref as masks_ref
import _change_ref as change_ref
import _gof_ref as gof_ref
import _presence_ref as presence_ref
import _refit_ref as refit_ref

SIGCHANGE_STREAM = 0x53430000
EPSILON = refit_ref.EPSILON
# the second counter words of every other draw: the resampler, the split, goodness of fit, and the families of 96 words each
OTHER_WORDS = ({0, 0x53504C54, gof_ref.GOF_STREAM} | {presence_ref.PRESENCE_STREAM + s for s in range(96)} | {0x50570000 + s for s in range(96)}
               | {change_ref.CHANGE_STREAM, change_ref.CHANGE_STREAM + 1})

# Largest deviations of the tied solve in two float64 feature orders from the longdouble one at FIXED steps on the inputs of
# tests/test_gpu_sigchange.py, measured on the CPU (tests/test_sigchange_host.py asserts that they hold); the device is held to
# 16 x these.
H_SPREAD = 1.5e-14  # measured 1.40e-14 (K = 96): |dh| / max(h_ld, EPSILON) on the candidate set, both sides
F_SPREAD = 2.1e-16  # measured 2.06e-16 (K = 3): |d f_a0|, |d f_b0| relative to the row's sum_v |x log(x / p)| + x + p
# The tie h_as / t_a = h_bs / t_b after n steps off the floor: each step multiplies both entries by the same F and rounds each
# product once, so the two shares part by at most one rounding per step and side, on top of the two divisions' own.
TIE_ROUNDINGS_PER_STEP = 2


def stream_word(s, side):
    return SIGCHANGE_STREAM + 2 * int(s) + int(side)


def pair_draw(h, W, T, n, s, side, b, seed):
    """Side ``side`` (0: a, 1: b) of null draw b of problem (n, s) from that side's tied exposures h with T trials -> float64 counts."""
    return presence_ref.draw_row(h, W, T, n, b, int(seed), stream_word(s, side)).astype(np.float64)


def draws_from(tied_a, tied_b, W, totals_a, totals_b, test, tested, n_draws, seed):
    """(B, N, S, 2, V): every tested problem's draws from the given tied exposures (N, S, K); zeros where untested."""
    N, S, _ = tied_a.shape
    out = np.zeros((n_draws, N, S, 2, W.shape[1]), dtype=np.float64)
    for n, j in zip(*np.nonzero(tested)):
        for b in range(n_draws):
            out[b, n, j, 0] = pair_draw(tied_a[n, j], W, totals_a[n], n, test[j], 0, b, seed)
            out[b, n, j, 1] = pair_draw(tied_b[n, j], W, totals_b[n], n, test[j], 1, b, seed)
    return out


def tested_problems(Xa, Xb, C, test):
    """(N, S) bool: s in C, at least two candidates and a positive total on either side."""
    return presence_ref.tested_pairs(C, test) & ((np.asarray(Xa).sum(axis=1) > 0) & (np.asarray(Xb).sum(axis=1) > 0))[:, None]


def tied_solve(Xa, Xb, W, C, s, min_iterations=500, max_iterations=10000, conv_test_freq=10, tol=1e-7, dtype=np.float64, perm=None, history=False):
    """The tied solve of every problem p: rows Xa[p], Xb[p] on the set C[p] with the share of signature s[p] tied.  With
    ``history`` nothing is latched before max_iterations, and the objective of every step and the last step's factors are kept."""
    Xa, Xb, W = np.asarray(Xa, dtype=np.float64), np.asarray(Xb, dtype=np.float64), np.asarray(W, dtype=np.float64)
    if perm is not None:
        Xa, Xb, W = Xa[:, perm], Xb[:, perm], W[:, perm]
    xa, xb, W = np.maximum(Xa, EPSILON).astype(dtype), np.maximum(Xb, EPSILON).astype(dtype), W.astype(dtype)
    P = xa.shape[0]
    C = np.asarray(C, dtype=bool)
    s = np.broadcast_to(np.asarray(s, dtype=np.int64), (P,))
    rows = np.arange(P)
    ta, tb = xa.sum(axis=1), xb.sum(axis=1)
    ca, cb = ta / (ta + tb), tb / (ta + tb)
    nc = C.sum(axis=1)
    ha = np.where(C, (ta / nc)[:, None], dtype(0.0)).astype(dtype)
    hb = np.where(C, (tb / nc)[:, None], dtype(0.0)).astype(dtype)
    stopped, conv = np.zeros(P, dtype=bool), np.zeros(P, dtype=bool)
    nit = np.zeros(P, dtype=np.int64)
    fa, fb, prev = np.zeros(P, dtype=dtype), np.zeros(P, dtype=dtype), np.zeros(P, dtype=dtype)
    objectives, factors = [], None
    it = 0
    while True:
        if it % conv_test_freq == 0 or history:
            cura, curb = refit_ref.objective(xa, W, ha), refit_ref.objective(xb, W, hb)
            cur = cura + curb
            if history:
                objectives.append(cur.copy())
            if it % conv_test_freq == 0:
                with np.errstate(invalid="ignore", divide="ignore"):
                    rel = np.abs(prev - cur) / np.abs(prev)
                hit = ~stopped & (it > 0) & (it >= min_iterations) & (rel < tol) & (not history)
                stop = hit | (~stopped & (it == max_iterations))
                conv |= hit
                fa[stop], fb[stop], nit[stop] = cura[stop], curb[stop], it
                prev = np.where(stopped, prev, cur)
                stopped |= stop
        if stopped.all():
            break
        ua, ub = masks_ref.update_factors(xa, W, ha), masks_ref.update_factors(xb, W, hb)
        F = 0.5 * (ua[rows, s] + ub[rows, s]) + (0.5 * (ca - cb)) * (ua[rows, s] - ub[rows, s])
        ua[rows, s], ub[rows, s] = F, F
        factors = (ua, ub)
        live = ~stopped[:, None]
        ha = np.where(live & (ha != 0.0), np.maximum(ha * ua, dtype(EPSILON)), ha)
        hb = np.where(live & (hb != 0.0), np.maximum(hb * ub, dtype(EPSILON)), hb)
        it += 1
    return SimpleNamespace(exposures_a=ha, exposures_b=hb, errors_a=fa, errors_b=fb, n_iterations=nit, converged=conv, totals_a=ta, totals_b=tb,
                           objectives=np.array(objectives), factors=factors)


def procedure(Xa, Xb, W, C, s, **kw):
    """The three solves of every row pair (all of them tested) -> namespace of the fits and the statistic."""
    a, b = presence_ref.solve(Xa, W, C, **kw), presence_ref.solve(Xb, W, C, **kw)
    tied = tied_solve(Xa, Xb, W, C, s, **kw)
    fa, fb = a.reconstruction_errors, b.reconstruction_errors
    return SimpleNamespace(a=a, b=b, tied=tied, statistic=(tied.errors_a - fa) + (tied.errors_b - fb))


def reduce_null(statistic, null_statistics):
    return presence_ref.reduce_null(statistic, null_statistics)


def signature_change(counts_a, counts_b, signatures, test, n_draws, seed=0, candidates=None, steps=300, fit=None):
    """The whole procedure on the host, at a fixed step count or under the iteration arguments ``fit``."""
    Xa, Xb = np.asarray(counts_a, dtype=np.float64), np.asarray(counts_b, dtype=np.float64)
    W = refit_ref.normalize(signatures)
    (N, V), K, B, S = Xa.shape, W.shape[0], n_draws, len(test)
    C = presence_ref.candidate_sets(candidates, N, K)
    tested = tested_problems(Xa, Xb, C, test)
    kw = dict(min_iterations=steps, max_iterations=steps) if fit is None else dict(fit)
    nan = np.nan
    res = SimpleNamespace(tested=tested, statistic=np.full((N, S), nan), exposures_a=np.full((N, K), nan), exposures_b=np.full((N, K), nan),
                          tied_exposures_a=np.full((N, S, K), nan), tied_exposures_b=np.full((N, S, K), nan), errors=np.full((N, S, 4), nan),
                          n_iterations=np.zeros((N, S, 3), dtype=np.int64), null_statistics=np.full((B, N, S), nan),
                          draws=np.zeros((B, N, S, 2, V)))
    ns, js = np.nonzero(tested)
    if ns.size:
        sig = np.asarray(test, dtype=np.int64)[js]
        obs = procedure(Xa[ns], Xb[ns], W, C[ns], sig, **kw)
        res.statistic[ns, js] = obs.statistic
        res.exposures_a[ns], res.exposures_b[ns] = obs.a.exposures, obs.b.exposures
        res.tied_exposures_a[ns, js], res.tied_exposures_b[ns, js] = obs.tied.exposures_a, obs.tied.exposures_b
        res.errors[ns, js] = np.stack([obs.a.reconstruction_errors, obs.b.reconstruction_errors, obs.tied.errors_a, obs.tied.errors_b], axis=1)
        res.n_iterations[ns, js] = np.stack([obs.a.dense.n_iterations, obs.b.dense.n_iterations, obs.tied.n_iterations], axis=1)
        res.draws = draws_from(res.tied_exposures_a, res.tied_exposures_b, W, Xa.sum(axis=1), Xb.sum(axis=1), test, tested, B, seed)
        drawn = res.draws[:, ns, js]  # (B, problems, 2, V)
        null = procedure(drawn[:, :, 0].reshape(-1, V), drawn[:, :, 1].reshape(-1, V), W, np.tile(C[ns], (B, 1)), np.tile(sig, B), **kw)
        res.null_statistics[:, ns, js] = null.statistic.reshape(B, ns.size)
    res.n_exceed, res.null_mean, res.p_value = reduce_null(res.statistic, res.null_statistics)
    return res


def dense_case(N=6, K=4, V=10, seed=5):
    """(counts (N, V), signatures (K, V)): rows without zeros under signatures without zeros -- nothing is clipped and nothing
    reaches the floor."""
    rng = np.random.default_rng(seed)
    W = refit_ref.normalize(rng.dirichlet(np.full(V, 2.0), size=K))
    E = rng.dirichlet(np.full(K, 1.0), size=N) * rng.uniform(200, 2000, size=(N, 1))
    return rng.poisson(E @ W).astype(np.float64) + 1.0, W


def row_scales(Xa, Xb, W, Ha, Hb):
    """sum_v |x log(x / p)| + x + p of the two rows at the given exposures."""
    return masks_ref.row_scale(Xa, W, Ha), masks_ref.row_scale(Xb, W, Hb)


CALIBRATION_SEED = 20241  # fixed before the first run; what the replica gives at it is in tests/test_sigchange_host.py
CALIBRATION_TEST = 0  # the tested signature: its common share in the null pairs is at least 0.1 by construction


def calibration_pairs(seed=CALIBRATION_SEED):
    """(counts_a (72, 96), counts_b (72, 96), catalogue (5, 96)), the catalogue built as ``_change_ref.calibration_pairs`` builds
    its own.  Pairs 0..63 are null: both rows are multinomial draws from one mixture of the five signatures, 2000 and 500
    mutations, in which signature 0 has a share of at least 0.1 (0.1 plus 0.9 of a flat Dirichlet draw).  Pairs 64..71 are planted
    in signature 4: a has shares 1/4 each on signatures 0-3, b half its mutations from signature 4 and the other half as a; both
    totals are 2000."""
    rng = np.random.default_rng(seed)
    V, K = 96, 5
    S = refit_ref.normalize(rng.dirichlet(np.full(V, 0.15), size=K))
    E = 0.9 * rng.dirichlet(np.full(K, 1.0), size=64)
    E[:, 0] += 0.1
    flat = np.array([0.25, 0.25, 0.25, 0.25, 0.0])
    Ea = np.vstack([E, np.tile(flat, (8, 1))])
    Eb = np.vstack([E, np.tile(0.5 * flat + np.array([0, 0, 0, 0, 0.5]), (8, 1))])
    Ta = np.full(72, 2000)
    Tb = np.r_[np.full(64, 500), np.full(8, 2000)]
    Xa = np.stack([rng.multinomial(t, p / p.sum()) for t, p in zip(Ta, Ea @ S)]).astype(np.float64)
    Xb = np.stack([rng.multinomial(t, p / p.sum()) for t, p in zip(Tb, Eb @ S)]).astype(np.float64)
    return Xa, Xb, S


# ---- the inputs of tests/test_gpu_sigchange.py, whose float64 spread tests/test_sigchange_host.py measures on the CPU: the pairs,
# catalogue and (N, K) mask of tests/_change_ref.py (row totals 0, 1, 2, 257 and 100 000, unequal inside pairs; the last signature
# row has zeros; pair 9 has one candidate), and per case tested signatures of the first and of the last 16-row tile.

GPU_N = change_ref.GPU_N
GPU_CASES = [(3, 7), (17, 96), (96, 96)]
GPU_TEST = {(3, 7): (0, 2), (17, 96): (3, 16, 9), (96, 96): (6, 95, 40)}  # 67, 91 and 95 tested problems: odd, several tiles of 8
GPU_FIT = change_ref.GPU_FIT  # the convergence rule: solves of one pair stop at different tests
GPU_FIXED = dict(min_iterations=40, max_iterations=40, conv_test_freq=10, tol=1e-5)  # every solve is 40 steps long
PERM_SEED = 7


def edge_test(K):
    """The tested signatures of a shape outside GPU_CASES: the first, bit 0 of the last candidate word and the last, K - 1."""
    return tuple(sorted({0, 32 * ((K - 1) // 32), K - 1}))


def gpu_case(K, V):
    """(counts_a, counts_b, signatures, candidates, test), never modified."""
    return (*change_ref.gpu_case(K, V), GPU_TEST[K, V] if (K, V) in GPU_TEST else edge_test(K))


@functools.lru_cache(maxsize=None)
def gpu_problems(K, V):
    """(ns, js, sig): the tested problems of a case, sample after sample."""
    Xa, Xb, W, C, test = gpu_case(K, V)
    ns, js = np.nonzero(tested_problems(Xa, Xb, C, test))
    return ns, js, np.asarray(test, dtype=np.int64)[js]


def deviations(got_a, got_b, got_fa, got_fb, ld, C, scale_a, scale_b):
    """(h, f) deviations of tied results from the longdouble run `ld`: |dh| / max(h_ld, EPSILON) on the set; |df| over the scales."""
    dh = 0.0
    for got, want in ((got_a, ld.exposures_a), (got_b, ld.exposures_b)):
        dh = max(dh, float((np.abs(got - want) / np.maximum(want, EPSILON))[C].max(initial=0.0)))
    df = max(float((np.abs(got_fa - ld.errors_a) / scale_a).max(initial=0.0)), float((np.abs(got_fb - ld.errors_b) / scale_b).max(initial=0.0)))
    return dh, df


@functools.lru_cache(maxsize=None)
def fixed_spread(K, V):
    """(H spread, f spread, longdouble run, scales) of the tied solve at GPU_FIXED on a case's tested problems."""
    Xa, Xb, W, C, _ = gpu_case(K, V)
    ns, _, sig = gpu_problems(K, V)
    perm = np.random.default_rng(PERM_SEED).permutation(V)
    ld = tied_solve(Xa[ns], Xb[ns], W, C[ns], sig, dtype=np.longdouble, **GPU_FIXED)
    scale_a, scale_b = row_scales(Xa[ns], Xb[ns], W, ld.exposures_a, ld.exposures_b)
    dh = df = 0.0
    for run in (tied_solve(Xa[ns], Xb[ns], W, C[ns], sig, **GPU_FIXED), tied_solve(Xa[ns], Xb[ns], W, C[ns], sig, perm=perm, **GPU_FIXED)):
        h, f = deviations(run.exposures_a, run.exposures_b, run.errors_a, run.errors_b, ld, C[ns], scale_a, scale_b)
        dh, df = max(dh, h), max(df, f)
    return dh, df, ld, (scale_a, scale_b)
