"""A NumPy replica of the device's model draw and of the goodness-of-fit reduction (``csrc/salnmf_gof.h``, DESIGN.md
section 16) -- TESTS ONLY.

Written from the contract, not from the kernel.  Row n of draw b, exposures h (K), signatures W (K, V), T trials:
    P = 0; for k ascending: P = P + h[k] * W[k]      (a rounded product, then a rounded sum: NumPy fuses nothing)
    S = 0; for v ascending: S = S + P[v];            S == 0, S not finite or T == 0: a zero row
    m_v = uint64(floor((P_v / S) * 2**40));  cum = prefix sums in uint64;  M = cum[V - 1]
    Philox4x32-10 (tests/_resample_ref.py), key (seed & 0xffffffff, seed >> 32), counter (q, 0x474F4644, n, b);
    draw 2q uses u = o0 | o1 << 32, draw 2q + 1 uses u = o2 | o3 << 32, draws j >= T are discarded;
    t = floor(u M / 2**64) -- the high half of the 128-bit product, from 32-bit limbs in uint64 (M < 2**47);
    the draw lands in the smallest v with cum[v] > t.
"""

import numpy as np

import _refit_ref as refit_ref
from _resample_ref import MASK, S32, philox4x32_10

GOF_STREAM = 0x474F4644
EPSILON = refit_ref.EPSILON


def spectrum(h, W):
    """(P, S) of the contract."""
    h, W = np.asarray(h, dtype=np.float64), np.asarray(W, dtype=np.float64)
    P = np.zeros(W.shape[1], dtype=np.float64)
    with np.errstate(invalid="ignore"):  # (an infinite exposure on a zero entry: NaN, S not finite, no draws)
        for k in range(W.shape[0]):
            P = P + h[k] * W[k]
    S = 0.0
    for v in range(P.size):
        S = S + float(P[v])
    return P, S


def weights(h, W):
    """(m, cum) as uint64 arrays, or None where the row has no draws whatever its total."""
    P, S = spectrum(h, W)
    if not (S > 0.0 and np.isfinite(S)):
        return None
    m = np.floor((P / S) * 2.0**40).astype(np.uint64)
    return m, np.cumsum(m, dtype=np.uint64)


def mulhi(ulo, uhi, M):
    """floor((ulo | uhi << 32) M / 2**64) for arrays of 32-bit words held in uint64 and a Python integer M < 2**64."""
    mlo, mhi = np.uint64(M & 0xFFFFFFFF), np.uint64(M >> 32)
    ll, lh, hl, hh = ulo * mlo, ulo * mhi, uhi * mlo, uhi * mhi
    mid = (ll >> S32) + (lh & MASK) + (hl & MASK)
    return hh + (lh >> S32) + (hl >> S32) + (mid >> S32)


def draw_row(h, W, T, n, b, seed, chunk=1 << 20):
    """One row of one draw -> int64 counts."""
    V = np.asarray(W).shape[1]
    out = np.zeros(V, dtype=np.int64)
    T = int(T)
    table = weights(h, W)
    if T == 0 or table is None:
        return out
    cum = table[1]
    M = int(cum[-1])
    k0, k1 = seed & 0xFFFFFFFF, seed >> 32
    n_blocks = (T + 1) // 2
    for start in range(0, n_blocks, chunk):
        q = np.arange(start, min(start + chunk, n_blocks), dtype=np.uint64)
        o0, o1, o2, o3 = philox4x32_10(q, np.full_like(q, GOF_STREAM), np.full_like(q, n), np.full_like(q, b), k0, k1)
        ulo = np.stack([o0, o2], axis=1).reshape(-1)  # draws 2q, 2q + 1
        uhi = np.stack([o1, o3], axis=1).reshape(-1)
        keep = 2 * int(q[0]) + np.arange(len(ulo)) < T
        t = mulhi(ulo[keep], uhi[keep], M)
        out += np.bincount(np.searchsorted(cum, t, side="right"), minlength=V)
    return out


def draw_model_counts(exposures, signatures, totals, n_draws, seed=0):
    """``(n_draws, N, V)`` float64 of integer values: what ``sal.draw_model_counts`` must return, entry for entry.  The
    signature rows are divided by their sums, as the product does."""
    H = np.asarray(exposures, dtype=np.float64)
    W = refit_ref.normalize(signatures)
    seed = int(seed)
    assert 0 <= seed < 2**64 and H.ndim == 2 and len(totals) == H.shape[0]
    out = np.zeros((n_draws, H.shape[0], W.shape[1]), dtype=np.float64)
    for b in range(n_draws):
        for n in range(H.shape[0]):
            out[b, n] = draw_row(H[n], W, totals[n], n, b, seed)
    return out


def reduce_null(err_obs, err_null):
    """(n_exceed, null_mean, p_value): comparisons in which a NaN is false, the sum in ascending b from 0.0, divided by B."""
    err_obs, err_null = np.asarray(err_obs, dtype=np.float64), np.asarray(err_null, dtype=np.float64)
    B, N = err_null.shape
    with np.errstate(invalid="ignore"):
        n_exceed = (err_null >= err_obs[None, :]).sum(axis=0).astype(np.int32)
    mean = np.array([sum((float(err_null[b, n]) for b in range(B)), 0.0) / B for n in range(N)])
    return n_exceed, mean, (1 + n_exceed.astype(np.int64)) / (B + 1)


def goodness_of_fit(counts, signatures, n_draws, seed=0, steps=300):
    """The whole procedure on the host at a fixed step count: observed refit, draws from its exposures, null refits, reduction."""
    X = np.asarray(counts, dtype=np.float64)
    W = refit_ref.normalize(signatures)
    kw = dict(min_iterations=steps, max_iterations=steps)
    obs = refit_ref.refit(X, W, **kw)
    drawn = draw_model_counts(obs.exposures, W, X.sum(axis=1), n_draws, seed)
    null = refit_ref.refit(drawn.reshape(-1, X.shape[1]), W, **kw)
    null_errors = null.reconstruction_errors.reshape(n_draws, X.shape[0])
    n_exceed, mean, p = reduce_null(obs.reconstruction_errors, null_errors)
    return obs, drawn, null_errors, n_exceed, mean, p


def calibration_samples():
    """The samples of the calibration tests, host and device: (counts (72, 96), catalogue (4, 96)).  Rows 0..63 are
    multinomial draws of 2000 mutations from mixtures of the catalogue's four signatures; rows 64..71 the same with 30 % of
    the mutations moved to a planted signature that the catalogue does not hold."""
    rng = np.random.default_rng(20240)
    V, K, T = 96, 4, 2000
    S = refit_ref.normalize(rng.dirichlet(np.full(V, 0.15), size=K + 1))
    catalogue, planted = S[:K], S[K]
    E = rng.dirichlet(np.full(K, 1.0), size=72)
    spectra = E @ catalogue
    spectra[64:] = 0.7 * spectra[64:] + 0.3 * planted
    X = np.stack([rng.multinomial(T, p / p.sum()) for p in spectra]).astype(np.float64)
    return X, catalogue
