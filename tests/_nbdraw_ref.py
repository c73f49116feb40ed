"""A NumPy replica of the device's negative-binomial model draw (``csrc/salnmf_nbdraw.h``) and of the
goodness-of-fit test built on it -- TESTS ONLY.

Written from the contract.  Row n of draw b, exposures h (K), signatures W (K, V), dispersion alpha, d = a' - 1/3 and
c = 1 / sqrt(9 d) with a' = alpha (alpha >= 1) or alpha + 1:
    1. P = spectrum(h, W) of tests/_gof_ref.py (a rounded product, then a rounded sum, ascending k);
    2. channel v < V with P_v / alpha != 0: gamma attempts q = 0 .. 63 on stream 0x4E420000 + v,
           block 2q:      u1 = u(o0, o1), u2 = u(o2, o3);  a_i = 2 u_i - 1;  s = a1 a1 + a2 a2;  rejected unless 0 < s < 1;
                          x = a1 sqrt((-2 log s) / s);  t = fma(c, x, 1);  v = (t t) t;  rejected unless v > 0;
           block 2q + 1:  u3 = u(o0, o1), u4 = u(o2, o3);  accepted iff log u3 < fma(d, log v, fma(-d, v, fma(0.5, x x, d)));
           g = d v, times exp(log(u4) / alpha) where alpha < 1;   lambda_v = g (P_v / alpha);
    3. Lambda = sum_v lambda_v from 0.0, ascending;  Lambda == 0 or not finite: a zero row;  Lambda >= 2**31: a failed row;
       T ~ Poisson(Lambda) on stream 0x4E42FF00 -- below 10: s = 0, for j = 0 .. 127: s = s - log u_j (u_j = u(o0, o1) or u(o2, o3)
       of block j >> 1), T = the first j with not (s < Lambda); from 10 on: PTRS, attempt q = 0 .. 63 from block q;
    4. T trials on stream 0x4E42FFFF over m_v = floor((lambda_v / Lambda) 2**40), placed as tests/_gof_ref.py places them.
    u(lo, hi) = (float(hi << 21 | lo >> 11) + 0.5) 2**-53.  A row that runs out of attempts is a failed row: zeros, and counted.
``log`` is ``log_pos`` (``_kl_ref.emu_log_pos``, here over arrays), ``exp`` and ``loggam`` are this file's, operation for operation
the header's; every fma is exact and rounded once (``fma`` below: an error-free product, an error-free sum, and a sum rounded
to odd in front of the final one -- Boldo and Melquiond 2008 -- so that it runs over arrays; tests/test_nbdraw_host.py holds it to
``_kl_ref.fma``).  A ``philox`` argument stands for the generator, so that a test can exhaust the attempt caps with a stub.
"""

from types import SimpleNamespace

import numpy as np

import _gof_ref as gof_ref
import _kl_ref as kl
import _nb_ref as nb_ref
from _resample_ref import philox4x32_10

NB_STREAM = 0x4E420000
NB_STREAM_TOTAL = 0x4E42FF00
NB_STREAM_PLACE = 0x4E42FFFF
GAMMA_ATTEMPTS, EXPONENTIALS, PTRS_ATTEMPTS = 64, 128, 64
EPSILON = gof_ref.EPSILON
LN2_HI, LN2_LO = 6.93147180369123816490e-01, 1.90821492927058770002e-10
INV_LN2 = 1.44269504088896338700e+00
EXP_COEFFS = [1.0 / 6227020800.0, 1.0 / 479001600.0, 1.0 / 39916800.0, 1.0 / 3628800.0, 1.0 / 362880.0, 1.0 / 40320.0, 1.0 / 5040.0, 1.0 / 720.0,
              1.0 / 120.0, 1.0 / 24.0, 1.0 / 6.0, 0.5, 1.0, 1.0]
LOGGAM_COEFFS = [-1.392432216905900e+00, 1.796443723688307e-01, -2.955065359477124e-02, 6.410256410256410e-03, -1.917526917526918e-03,
                 8.417508417508418e-04, -5.952380952380952e-04, 7.936507936507937e-04, -2.777777777777778e-03, 8.333333333333333e-02]
HALF_LOG_2PI = 9.189385332046727e-01


def _two_sum(a, b):
    s = a + b
    bb = s - a
    return s, (a - (s - bb)) + (b - bb)


def fma(a, b, c):
    """a b + c rounded once, over arrays (no overflow, no subnormal intermediate: the sampler's operands)."""
    a, b, c = (np.asarray(v, dtype=np.float64) for v in np.broadcast_arrays(a, b, c))
    with np.errstate(invalid="ignore", over="ignore"):
        uh = a * b
        t = 134217729.0 * a
        ah = t - (t - a)
        al = a - ah
        t = 134217729.0 * b
        bh = t - (t - b)
        bl = b - bh
        ul = ((ah * bh - uh) + ah * bl + al * bh) + al * bl
        th, tl = _two_sum(c, uh)
        v, e = _two_sum(tl, ul)
        even = (np.ascontiguousarray(v).view(np.int64) & 1) == 0
        v = np.where((e != 0) & even, np.nextafter(v, np.where(e > 0, np.inf, -np.inf)), v)  # tl + ul rounded to odd
        out = th + v
        plain = a * b + c
    return np.where(np.isfinite(out), out, plain)  # (an infinite operand: the plain expression is the answer)


def log_pos(p):
    """``log_pos_n`` (salnmf_kernels.h) over an array of positive normal doubles, as ``_kl_ref.emu_log_pos`` does for one."""
    inv, lc = kl._TAB()
    p = np.ascontiguousarray(p, dtype=np.float64)
    i = ((p.view(np.int64) >> 32) >> 12) & 0xFF
    m, e = np.frexp(p)
    kd = e.astype(np.float64)
    r = fma(m, inv[i], -1.0)
    r2 = r * r
    h = fma(r, 0.2, -0.25)
    h = fma(r, h, 0.33333333333333331)
    h = fma(r, h, -0.5)
    h = fma(r2, h, r)
    u = fma(kd, LN2_HI, lc[i])
    h = fma(kd, LN2_LO, h)
    return u + h


def nb_exp(t):
    t = np.asarray(t, dtype=np.float64)
    safe = np.where(t < -708.0, 0.0, t)
    kd = (safe * INV_LN2 + 6755399441055744.0) - 6755399441055744.0  # 1.5 x 2**52: the sum rounds to the nearest integer
    r = fma(-kd, LN2_HI, safe)
    r = fma(-kd, LN2_LO, r)
    p = np.full(t.shape, EXP_COEFFS[0])
    for coeff in EXP_COEFFS[1:]:
        p = fma(p, r, coeff)
    return np.where(t < -708.0, 0.0, np.ldexp(p, kd.astype(np.int64)))


def nb_loggam(x):
    x = np.asarray(x, dtype=np.float64)
    nd = np.where(x < 7.0, 7.0 - x, 0.0)
    x0 = x + nd
    prod = np.ones(x.shape)
    for i in range(6):
        prod = np.where(float(i) < nd, prod * (x + float(i)), prod)
    x2 = 1.0 / (x0 * x0)
    g = np.full(x.shape, LOGGAM_COEFFS[0])
    for coeff in LOGGAM_COEFFS[1:]:
        g = fma(g, x2, coeff)
    tail = fma(x0 - 0.5, log_pos(x0), -x0)
    gl = (g / x0 + HALF_LOG_2PI) + tail
    return np.where(nd > 0.0, gl - log_pos(prod), gl)


def uniform(lo, hi):
    return ((((hi << np.uint64(21)) | (lo >> np.uint64(11))).astype(np.float64)) + 0.5) * 2.0**-53


def gamma_constants(alpha):
    alpha = np.asarray(alpha, dtype=np.float64)
    d = np.where(alpha >= 1.0, alpha, alpha + 1.0) - 1.0 / 3.0
    return d, 1.0 / np.sqrt(9.0 * d)


def _blocks(philox, q, stream, n, b, seed):
    shape = np.broadcast(q, stream, n, b).shape
    words = [np.broadcast_to(np.asarray(w, dtype=np.uint64), shape).copy() for w in (q, stream, n, b)]
    return philox(*words, seed & 0xFFFFFFFF, seed >> 32)


def gamma(alpha, stream, n, b, seed, philox=philox4x32_10):
    """(g, ok) for arrays of lanes: the dispersion, the stream word, the row and the draw of each."""
    alpha = np.asarray(alpha, dtype=np.float64)
    d, c = gamma_constants(alpha)
    stream, n, b = (np.broadcast_to(np.asarray(w, dtype=np.uint64), alpha.shape) for w in (stream, n, b))
    g = np.zeros(alpha.shape)
    live = np.arange(alpha.size)
    for q in range(GAMMA_ATTEMPTS):
        if live.size == 0:
            break
        o = _blocks(philox, 2 * q, stream[live], n[live], b[live], seed)
        a1 = 2.0 * uniform(o[0], o[1]) - 1.0
        a2 = 2.0 * uniform(o[2], o[3]) - 1.0
        s = a1 * a1 + a2 * a2
        keep = (s > 0.0) & (s < 1.0)
        live2, a1, s = live[keep], a1[keep], s[keep]
        x = a1 * np.sqrt((-2.0 * log_pos(s)) / s)
        t = fma(c[live2], x, 1.0)
        v = (t * t) * t
        keep = v > 0.0
        live2, x, v = live2[keep], x[keep], v[keep]
        o = _blocks(philox, 2 * q + 1, stream[live2], n[live2], b[live2], seed)
        dl = d[live2]
        rhs = fma(dl, log_pos(v), fma(-dl, v, fma(0.5, x * x, dl)))
        keep = log_pos(uniform(o[0], o[1])) < rhs
        done, v = live2[keep], v[keep]
        out = d[done] * v
        small = alpha[done] < 1.0
        boost = nb_exp(log_pos(uniform(o[2][keep], o[3][keep])) / alpha[done])
        g[done] = np.where(small, out * boost, out)
        live = np.setdiff1d(live, done, assume_unique=True)
    ok = np.ones(alpha.shape, dtype=bool)
    ok[live] = False
    return g, ok


def _one(v):
    return np.array([v], dtype=np.float64)


def _f(v):
    return float(np.asarray(v).reshape(-1)[0])


def poisson(lam, n, b, seed, philox=philox4x32_10):
    """(T, ok) for one row, 0 < lam < 2**31."""
    lam = float(lam)
    if lam < 10.0:
        s = 0.0
        for j in range(EXPONENTIALS):
            if j % 2 == 0:
                o = _blocks(philox, j >> 1, NB_STREAM_TOTAL, n, b, seed)
            u = uniform(o[2], o[3]) if j % 2 else uniform(o[0], o[1])
            s = s - float(log_pos(u.reshape(1))[0])
            if not s < lam:
                return j, True
        return 0, False
    slam, loglam = float(np.sqrt(lam)), float(log_pos(_one(lam))[0])
    bb = _f(fma(2.53, slam, 0.931))
    aa = _f(fma(0.02483, bb, -0.059))
    invalpha = 1.1239 + 1.1328 / (bb - 3.4)
    vr = 0.9277 - 3.6224 / (bb - 2.0)
    log_invalpha, shifted = float(log_pos(_one(invalpha))[0]), lam + 0.43
    for q in range(PTRS_ATTEMPTS):
        o = _blocks(philox, q, NB_STREAM_TOTAL, n, b, seed)
        U = float(uniform(o[0], o[1]).reshape(1)[0]) - 0.5
        Vv = float(uniform(o[2], o[3]).reshape(1)[0])
        us = 0.5 - abs(U)
        if not us > 0.0:
            continue
        k = _f(np.floor(fma((2.0 * aa) / us + bb, U, shifted)))
        accept = us >= 0.07 and Vv <= vr
        if not accept:
            if k < 0.0 or (us < 0.013 and Vv > us):
                continue
            lhs = (float(log_pos(_one(Vv))[0]) + log_invalpha) - float(log_pos(_one(aa / (us * us) + bb))[0])
            if not k < 4294967296.0:
                continue
            accept = lhs <= _f(fma(k, loglam, -lam)) - _f(nb_loggam(_one(k + 1.0)))
        if accept:
            if not (0.0 <= k < 4294967296.0):
                return 0, False
            return int(k), True
    return 0, False


def place(lam_row, L, T, n, b, seed, philox=philox4x32_10, chunk=1 << 20):
    """T trials over the 40-bit table of lam_row / L, as ``_gof_ref.draw_row`` places them, on the placement stream."""
    V = lam_row.size
    out = np.zeros(V, dtype=np.int64)
    cum = np.cumsum(np.floor((lam_row / L) * 2.0**40).astype(np.uint64), dtype=np.uint64)
    M = int(cum[-1])
    n_blocks = (T + 1) // 2
    for start in range(0, n_blocks, chunk):
        q = np.arange(start, min(start + chunk, n_blocks), dtype=np.uint64)
        o0, o1, o2, o3 = _blocks(philox, q, NB_STREAM_PLACE, n, b, seed)
        ulo = np.stack([o0, o2], axis=1).reshape(-1)
        uhi = np.stack([o1, o3], axis=1).reshape(-1)
        keep = 2 * int(q[0]) + np.arange(len(ulo)) < T
        out += np.bincount(np.searchsorted(cum, gof_ref.mulhi(ulo[keep], uhi[keep], M), side="right"), minlength=V)
    return out


def rates(H, W, alpha, rows, b, seed, philox=philox4x32_10):
    """(lambda (R, V), ok (R,)) of the rows ``rows`` (their counter words) of draw b (one word, or one per row): steps 1 and 2 for
    all lanes at once."""
    H, W = np.asarray(H, dtype=np.float64), np.asarray(W, dtype=np.float64)
    R, V = H.shape[0], W.shape[1]
    alpha = np.broadcast_to(np.asarray(alpha, dtype=np.float64), (R,))
    P = np.zeros((R, V))
    for k in range(W.shape[0]):  # _gof_ref.spectrum over the rows: a rounded product, then a rounded sum
        P = P + H[:, k:k + 1] * W[k]
    scale = P / alpha[:, None]
    r_idx, v_idx = np.nonzero(scale != 0.0)
    g, ok = gamma(alpha[r_idx], NB_STREAM + v_idx, np.asarray(rows)[r_idx], np.broadcast_to(np.asarray(b), (R,))[r_idx], seed, philox)
    G = np.zeros((R, V))
    G[r_idx, v_idx] = g
    good = np.ones(R, dtype=bool)
    good[r_idx[~ok]] = False
    return G * scale, good


def draw_nb_counts(exposures, signatures, dispersion, n_draws, seed=0, rows=None, draws=None, philox=philox4x32_10, normalize=True):
    """``((n_draws, N, V) float64 of integer values, n_failed)``: what ``sal.draw_nb_counts`` must return, entry for entry.
    ``rows`` are the rows' counter words (default 0 .. N - 1), ``draws`` the draws' (default 0 .. n_draws - 1)."""
    H = np.asarray(exposures, dtype=np.float64)
    W = gof_ref.refit_ref.normalize(signatures) if normalize else np.asarray(signatures, dtype=np.float64)
    seed = int(seed)
    N, V = H.shape[0], W.shape[1]
    rows = np.arange(N) if rows is None else np.asarray(rows)
    draws = list(range(n_draws)) if draws is None else list(draws)
    alpha = np.broadcast_to(np.asarray(dispersion, dtype=np.float64), (N,))
    out = np.zeros((len(draws), N, V), dtype=np.float64)
    failed = 0
    # steps 1 and 2 for every lane of every (draw, row) at once; then row by row
    lam_all, ok_all = rates(np.tile(H, (len(draws), 1)), W, np.tile(alpha, len(draws)), np.tile(rows, len(draws)), np.repeat(draws, N), seed, philox)
    for i, b in enumerate(draws):
        lam, ok = lam_all[i * N:(i + 1) * N], ok_all[i * N:(i + 1) * N]
        for r in range(N):
            L = 0.0
            for v in range(V):
                L = L + float(lam[r, v])
            if not ok[r]:
                failed += 1
                continue
            if not (L > 0.0 and np.isfinite(L)):
                continue
            T, fine = poisson(L, int(rows[r]), b, seed, philox) if L < 2147483648.0 else (0, False)
            if not fine:
                failed += 1
            elif T:
                out[i, r] = place(lam[r], L, T, int(rows[r]), b, seed, philox)
    return out, failed


def nb_goodness_of_fit(counts, signatures, dispersion, n_draws, seed=0, steps=300, **kw):
    """The whole procedure on the host: observed NB refit, draws from its exposures, null refits, reduction.  A fixed step count
    unless iteration keywords are given."""
    X = np.asarray(counts, dtype=np.float64)
    W = gof_ref.refit_ref.normalize(signatures)
    kw = kw or dict(min_iterations=steps, max_iterations=steps)
    alpha = np.broadcast_to(np.asarray(dispersion, dtype=np.float64), (X.shape[0],))
    obs = nb_ref.nb_refit(X, W, alpha, **kw)
    drawn, failed = draw_nb_counts(obs.exposures, W, alpha, n_draws, seed, normalize=False)
    assert failed == 0
    null = nb_ref.nb_refit(drawn.reshape(-1, X.shape[1]), W, np.tile(alpha, n_draws), **kw)
    null_errors = null.reconstruction_errors.reshape(n_draws, X.shape[0])
    n_exceed, mean, p = gof_ref.reduce_null(obs.reconstruction_errors, null_errors)
    return SimpleNamespace(obs=obs, draws=drawn, null=null, null_errors=null_errors, n_exceed=n_exceed, null_mean=mean, p_value=p)


def calibration_samples():
    """The samples of the calibration tests, host and device: (counts (72, 96), catalogue (4, 96), alpha = 20).  Rows 0..63 are
    gamma-Poisson counts (alpha = 20, K = 4, V = 96, about 2000 mutations) around mixtures of the catalogue's four signatures; rows
    64..71 the same with 30 % of the mean moved to a planted signature that the catalogue does not hold."""
    rng = np.random.default_rng(20241)
    V, K, mu, alpha = 96, 4, 2000.0, 20.0
    S = gof_ref.refit_ref.normalize(rng.dirichlet(np.full(V, 0.15), size=K + 1))
    catalogue, planted = S[:K], S[K]
    E = rng.dirichlet(np.full(K, 1.0), size=72)
    spectra = E @ catalogue
    spectra[64:] = 0.7 * spectra[64:] + 0.3 * planted
    M = mu * spectra
    X = rng.poisson(M * rng.gamma(alpha, 1.0 / alpha, size=M.shape)).astype(np.float64)
    return X, catalogue, alpha


DISPERSION_TEST = dict(N=16, K=3, V=96, mu=2000.0, alpha=20.0, B=19, grid=np.geomspace(1, 1e4, 5))
DISPERSION_TEST_SEED = 0  # of the data (tests/_nb_ref.py: gamma_poisson_catalogue) and of the draws


def dispersion_test_data(poisson=False):
    c = DISPERSION_TEST
    X, W, _ = nb_ref.gamma_poisson_catalogue(c["N"], c["K"], c["V"], seed=DISPERSION_TEST_SEED, mu=c["mu"], alpha=None if poisson else c["alpha"])
    return X, W


def dispersion_test(counts, signatures, grid, n_draws, seed=0, steps=300):
    """``sal.dispersion_test`` for the cohort on the host at a fixed step count: the estimate, the Poisson-null p-value of
    ``lr_statistic`` and the estimates on cohorts drawn from the NB fit at the estimate."""
    X = np.asarray(counts, dtype=np.float64)
    W = gof_ref.refit_ref.normalize(signatures)
    grid = np.asarray(grid, dtype=np.float64)
    kw = dict(min_iterations=steps, max_iterations=steps)
    (N, V), K, A = X.shape, W.shape[0], grid.size

    def estimate(Y):
        profile, poisson_ll, fit = nb_ref.dispersion_profile(Y, W, grid, **kw)
        return nb_ref.select(grid, profile, poisson_ll) + (fit,)

    a_hat, edge, lr, fit = estimate(X)
    pois = gof_ref.refit_ref.refit(X, W, **kw)
    null = gof_ref.draw_model_counts(pois.exposures, W, X.sum(axis=1), n_draws, seed)
    null_lr = np.array([estimate(null[b])[2] for b in range(n_draws)])
    H = np.asarray(fit.exposures).reshape(A, N, K)[int(np.searchsorted(grid, a_hat))]
    drawn, failed = draw_nb_counts(H, W, a_hat, n_draws, seed, normalize=False)
    assert failed == 0
    draws = np.array([estimate(drawn[b])[0] for b in range(n_draws)])
    return SimpleNamespace(dispersion=a_hat, at_upper_edge=edge, lr_statistic=lr, null_lr=null_lr, p_value=(1 + int((null_lr >= lr).sum())) / (n_draws + 1),
                           dispersion_draws=draws, dispersion_bias=float(np.median(draws)) / a_hat)
