"""A NumPy replica of ``sal.exposure_change_test`` (``csrc/salnmf_change.h``) -- TESTS ONLY.

Written from the contract, on ``_presence_ref`` (the solve on a set, the draw under a stream word), ``_gof_ref`` (the reduction)
and ``_assign_masks_ref``.  For pair n with clipped rows x_a, x_b and candidate set C, |C| >= 2, both integer totals positive:
    solves a, b and pooled: ``_presence_ref.solve`` of x_a, of x_b and of x_p = x_a + x_b on C -> (h_a, f_a), (h_b, f_b), (h_0, f_p);
    c_a = t_a / (t_a + t_b), c_b = t_b / (t_a + t_b) with t the rows' sums;  P_0 = h_0 W;
    g_a = KL(x_a || c_a P_0), g_b = KL(x_b || c_b P_0);  statistic = (g_a - f_a) + (g_b - f_b);
    null draw b: two model draws from h_0 with T_a and T_b trials under the Philox counter (q, 0x43480000 + side, n, b);
    every draw pair goes through the same steps -> t_b;  the reduction is ``_gof_ref.reduce_null``.
The identity g_a + g_b - f_p = D, D = sum_v [x_a ln(x_a / (c_a x_p)) + x_b ln(x_b / (c_b x_p))], holds for ANY P_0: the
-x + p terms cancel because c_a + c_b = 1, the logarithms of P_0 because x_a + x_b = x_p.  D is the G statistic of the 2 x V table.
"""

import functools
from types import SimpleNamespace

import numpy as np

import _gof_ref as gof_ref
import _presence_ref as presence_ref
import _refit_ref as refit_ref

CHANGE_STREAM = 0x43480000
EPSILON = refit_ref.EPSILON
OTHER_STREAMS = {"resample": 0, "split": 0x53504C54, "gof": gof_ref.GOF_STREAM, "presence": presence_ref.PRESENCE_STREAM, "power": 0x50570000}

# Largest deviations of float64 evaluations from the longdouble one, measured on the CPU (tests/test_change_host.py asserts that
# they hold); the device is held to 16 x G_SPREAD.  Both are relative to the row's sum_v |x log(x / p)| + x + p over the
# divergences that enter.
IDENTITY_BOUND = 8.5e-16  # 16 x the measured 5.2e-17: |(g_a + g_b - f_p) - D| on the replica at 30 and 300 steps (identity_cases)
G_SPREAD = 1.5e-16  # measured 1.48e-16 (K = 96): g_a, g_b in two float64 feature orders against longdouble on the cases of tests/test_gpu_change.py


def pair_draw(h0, W, T, n, side, b, seed):
    """Side ``side`` (0: a, 1: b) of null draw b of pair n from the pooled fit's exposures h0 with T trials -> float64 counts."""
    return presence_ref.draw_row(h0, W, T, n, b, int(seed), CHANGE_STREAM + int(side)).astype(np.float64)


def draws_from(pooled_exposures, W, totals_a, totals_b, tested, n_draws, seed):
    """(B, N, 2, V): every tested pair's draws from the given pooled exposures (N, K); zeros where the pair is untested."""
    N = pooled_exposures.shape[0]
    out = np.zeros((n_draws, N, 2, W.shape[1]), dtype=np.float64)
    for n in np.flatnonzero(tested):
        for b in range(n_draws):
            out[b, n, 0] = pair_draw(pooled_exposures[n], W, totals_a[n], n, 0, b, seed)
            out[b, n, 1] = pair_draw(pooled_exposures[n], W, totals_b[n], n, 1, b, seed)
    return out


def tested_pairs(Xa, Xb, C):
    """(N,) bool: at least two candidates and a positive total on either side."""
    return (C.sum(axis=1) > 1) & (np.asarray(Xa).sum(axis=1) > 0) & (np.asarray(Xb).sum(axis=1) > 0)


def null_divergences(Xa, Xb, W, H0, dtype=np.float64, perm=None):
    """(g_a, g_b, scale_a, scale_b) of every row at the pooled exposures H0; the scales are sum_v |x log(x / p)| + x + p."""
    W = np.asarray(W, dtype=np.float64)
    Xa, Xb = np.asarray(Xa, dtype=np.float64), np.asarray(Xb, dtype=np.float64)
    if perm is not None:
        Xa, Xb, W = Xa[:, perm], Xb[:, perm], W[:, perm]
    xa, xb = np.maximum(Xa, EPSILON).astype(dtype), np.maximum(Xb, EPSILON).astype(dtype)
    P0 = refit_ref._wh(np.asarray(H0).astype(dtype), W.astype(dtype))
    ta, tb = xa.sum(axis=1), xb.sum(axis=1)
    out = []
    for x, t in ((xa, ta), (xb, tb)):
        p = (t / (ta + tb))[:, None] * P0
        term = x * np.log(x / p)
        out.append(((term - x + p).sum(axis=1), (np.abs(term) + x + p).sum(axis=1)))
    return out[0][0], out[1][0], out[0][1], out[1][1]


def table_statistic(Xa, Xb):
    """D of the module docstring in longdouble, and the scale sum_v |x_a ln(.)| + |x_b ln(.)|."""
    xa, xb = np.maximum(Xa, EPSILON).astype(np.longdouble), np.maximum(Xb, EPSILON).astype(np.longdouble)
    xp = xa + xb
    ta, tb = xa.sum(axis=1), xb.sum(axis=1)
    ca, cb = (ta / (ta + tb))[:, None], (tb / (ta + tb))[:, None]
    ea, eb = xa * np.log(xa / (ca * xp)), xb * np.log(xb / (cb * xp))
    return (ea + eb).sum(axis=1), (np.abs(ea) + np.abs(eb)).sum(axis=1)


def procedure(Xa, Xb, W, C, **kw):
    """Steps 1-5 of the contract on every row (all of them tested) -> namespace of the three fits, g_a, g_b and the statistic."""
    xa, xb = np.maximum(Xa, EPSILON), np.maximum(Xb, EPSILON)
    a, b, p = presence_ref.solve(Xa, W, C, **kw), presence_ref.solve(Xb, W, C, **kw), presence_ref.solve(xa + xb, W, C, **kw)
    ga, gb, _, _ = null_divergences(Xa, Xb, W, p.exposures)
    fa, fb = a.reconstruction_errors, b.reconstruction_errors
    return SimpleNamespace(a=a, b=b, pooled=p, ga=ga, gb=gb, statistic=(ga - fa) + (gb - fb))


def reduce_null(statistic, null_statistics):
    """(n_exceed, null_mean, p_value) of (N,) and (B, N) by the stated rules; NaN p where the statistic is NaN."""
    n_exceed, mean, p = gof_ref.reduce_null(statistic, null_statistics)
    return n_exceed, mean, np.where(np.isnan(statistic), np.nan, p)


def change(counts_a, counts_b, signatures, n_draws, seed=0, candidates=None, steps=300):
    """The whole procedure on the host at a fixed step count."""
    Xa, Xb = np.asarray(counts_a, dtype=np.float64), np.asarray(counts_b, dtype=np.float64)
    W = refit_ref.normalize(signatures)
    (N, V), K, B = Xa.shape, W.shape[0], n_draws
    C = presence_ref.candidate_sets(candidates, N, K)
    tested = tested_pairs(Xa, Xb, C)
    kw = dict(min_iterations=steps, max_iterations=steps)
    nan = np.nan
    res = SimpleNamespace(tested=tested, statistic=np.full(N, nan), exposures_a=np.full((N, K), nan), exposures_b=np.full((N, K), nan),
                          pooled_exposures=np.full((N, K), nan), errors=np.full((N, 3), nan), null_errors=np.full((N, 2), nan),
                          null_statistics=np.full((B, N), nan), draws=np.zeros((B, N, 2, V)))
    rows = np.flatnonzero(tested)
    if rows.size:
        obs = procedure(Xa[rows], Xb[rows], W, C[rows], **kw)
        res.statistic[rows] = obs.statistic
        res.exposures_a[rows], res.exposures_b[rows], res.pooled_exposures[rows] = obs.a.exposures, obs.b.exposures, obs.pooled.exposures
        res.errors[rows] = np.stack([obs.a.reconstruction_errors, obs.b.reconstruction_errors, obs.pooled.reconstruction_errors], axis=1)
        res.null_errors[rows] = np.stack([obs.ga, obs.gb], axis=1)
        res.draws = draws_from(res.pooled_exposures, W, Xa.sum(axis=1), Xb.sum(axis=1), tested, B, seed)
        drawn = res.draws[:, rows]
        null = procedure(drawn[:, :, 0].reshape(-1, V), drawn[:, :, 1].reshape(-1, V), W, np.tile(C[rows], (B, 1)), **kw)
        res.null_statistics[:, rows] = null.statistic.reshape(B, rows.size)
    res.n_exceed, res.null_mean, res.p_value = reduce_null(res.statistic, res.null_statistics)
    return res


def identity_cases():
    """(counts_a, counts_b, signatures, steps) of the identity test: 12 pairs, K = 4, V = 10, b at about a third of a's total."""
    for seed, steps in ((0, 30), (3, 300)):
        Xa, W = refit_ref.poisson_catalogue(12, 4, V=10, seed=seed, mutations=(50, 4000))
        Xb = np.random.default_rng(seed).poisson(0.3 * Xa.mean(axis=1, keepdims=True) * np.ones_like(Xa)).astype(np.float64)
        Xa[:, 1] += 1
        Xb[:, 0] += 1
        yield Xa, Xb, W, steps


CALIBRATION_SEED = 20240  # the issue's generator seed: both conditions hold on the replica at it (tests/test_change_host.py)


def calibration_pairs(seed=CALIBRATION_SEED):
    """(counts_a (72, 96), counts_b (72, 96), catalogue (5, 96)), the catalogue built as ``_gof_ref.calibration_samples`` builds
    its own.  Pairs 0..63 are null: both rows are multinomial draws from one mixture of the five signatures, 2000 and 500
    mutations.  Pairs 64..71 are planted: a has shares 1/4 each on signatures 0-3, b half its mutations from signature 4 and the
    other half as a; both totals are 2000."""
    rng = np.random.default_rng(seed)
    V, K = 96, 5
    S = refit_ref.normalize(rng.dirichlet(np.full(V, 0.15), size=K))
    E = rng.dirichlet(np.full(K, 1.0), size=64)
    flat = np.array([0.25, 0.25, 0.25, 0.25, 0.0])
    Ea = np.vstack([E, np.tile(flat, (8, 1))])
    Eb = np.vstack([E, np.tile(0.5 * flat + np.array([0, 0, 0, 0, 0.5]), (8, 1))])
    Ta = np.full(72, 2000)
    Tb = np.r_[np.full(64, 500), np.full(8, 2000)]
    Xa = np.stack([rng.multinomial(t, p / p.sum()) for t, p in zip(Ta, Ea @ S)]).astype(np.float64)
    Xb = np.stack([rng.multinomial(t, p / p.sum()) for t, p in zip(Tb, Eb @ S)]).astype(np.float64)
    return Xa, Xb, S


# ---- the inputs of tests/test_gpu_change.py, whose float64 spread tests/test_change_host.py measures on the CPU

GPU_N = 40  # two full tiles of 16 problems and a partial one
GPU_CASES = [(1, 7), (3, 7), (17, 96), (96, 96)]
GPU_FIT = dict(min_iterations=20, max_iterations=60, conv_test_freq=10, tol=1e-5)
PERM_SEED = 7


@functools.lru_cache(maxsize=None)
def gpu_case(K, V):
    """(counts_a, counts_b, signatures, candidates), computed once and never modified: Poisson counts of unequal totals from one
    catalogue, three zero-heavy rows in a; row totals (a, b) of pairs 0..5: (0, *), (1, 257), (2, 1), (257, 100 000), (100 000, 2),
    (*, 0); the last signature row has zeros (row a of pair 3 is drawn from it); an (N, K) mask in which pair 9 holds the dense
    signature 1 alone, and every other set holds it too, so that no feature with counts is left without a signature.

    A shape outside GPU_CASES (tests/test_gpu_family_edges.py) gets the candidate-word edge as well: every set but pair 9's also
    holds signature K - 1 and signature 32 floor((K - 1) / 32).  The cases of GPU_CASES are what they were."""
    N = GPU_N
    rng = np.random.default_rng(1000 * K + V)
    Xa, W = refit_ref.poisson_catalogue(N, K, V=V, seed=70 + K, zero_heavy=3)
    W[K - 1, rng.permutation(V)[: min(max(2, V // 3), V - 1)]] = 0.0  # (the last signature keeps a feature at any V)
    W = refit_ref.normalize(W)
    E = rng.dirichlet(np.full(K, 0.3), size=N) * rng.uniform(50, 3000, size=(N, 1))
    Xb = rng.poisson(E @ W).astype(np.float64)
    uniform = np.full(V, 1.0 / V)
    for row, (ta, tb) in enumerate(((0, None), (1, 257), (2, 1), (257, 100000), (100000, 2), (None, 0))):
        if ta is not None:
            Xa[row] = rng.multinomial(ta, W[K - 1] if row == 3 else uniform)
        if tb is not None:
            Xb[row] = rng.multinomial(tb, uniform)
    C = rng.random((N, K)) < 0.8
    C[:, min(1, K - 1)] = True
    if (K, V) not in GPU_CASES:
        C[:, [K - 1, 32 * ((K - 1) // 32)]] = True
    C[:9] = True
    C[9] = False
    C[9, min(1, K - 1)] = True
    for X in (Xa, Xb, W, C):
        X.setflags(write=False)
    return Xa, Xb, W, C


def g_spread(K, V):
    """The largest deviation of g_a, g_b in two float64 feature orders from the longdouble evaluation, relative to the row's scale,
    on a case's tested pairs at the replica's own pooled exposures (the convergence rule of the device test)."""
    Xa, Xb, W, C = gpu_case(K, V)
    rows = np.flatnonzero(tested_pairs(Xa, Xb, C))
    if not rows.size:
        return 0.0
    xa, xb = np.maximum(Xa[rows], EPSILON), np.maximum(Xb[rows], EPSILON)
    H0 = presence_ref.solve(xa + xb, W, C[rows], **GPU_FIT).exposures
    perm = np.random.default_rng(PERM_SEED).permutation(V)
    ld = null_divergences(Xa[rows], Xb[rows], W, H0, dtype=np.longdouble)
    worst = 0.0
    for run in (null_divergences(Xa[rows], Xb[rows], W, H0), null_divergences(Xa[rows], Xb[rows], W, H0, perm=perm)):
        for side in (0, 1):
            worst = max(worst, float((np.abs(run[side] - ld[side]) / ld[2 + side]).max()))
    return worst
