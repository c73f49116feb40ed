"""Reference and error model of the fp32 fast mode's joint KL step (``salnmf_kernels_f32.h``), NumPy only.

The step, as the kernel's header defines it (sample-major ``X (N, V)``, ``W (K, V)``, ``H (N, K)``)::

    X32 = float32(X), H32 = float32(H), W32 = float32(W)          the shadow copies and the LDS images of W
    P = H32 W32,  R = X32 / P,  U = R W32^T,  G = H32^T R          fp32 matrix cores
    H' = max(H32 * U, float32(EPSILON))                            written as float32, handed back as float64
    W' = clip(normalise(W * G), EPSILON), given rows kept          the fp64 tail of the default path, on the UNROUNDED W

:func:`exact_step` evaluates exactly this in ``np.longdouble``: it is what the device would return if every fp32
operation were exact, so the distance of the device from it is the kernel's own rounding and nothing else (the rounding
of the inputs is part of the definition, not of the error).  :func:`replica_step` is the same step in float32 NumPy in two
summation orders; it shows on the host how much of the bound real fp32 arithmetic uses.

The bound
---------
Every sum of the step is a sum of non-negative terms (counts, signatures and exposures are >= 0), so a relative error
of each term bounds the relative error of the sum: no cancellation anywhere.  ``u = 2^-24`` is the unit roundoff of
fp32 under round-to-nearest; ``(1 + u)^n <= 1 + n u (1 + n u)`` and ``n <= 200`` here, so second-order terms stay below
``1e-5 u`` per factor and are covered by the slack named below.  Assumptions: (i) every fp32 product and sum, inside
``v_mfma_f32_16x16x4_f32`` too, is rounded once, to nearest -- in ANY order of the additions; (ii) ``v_rcp_f32`` is good
to 1 ulp (the kernel's comment), i.e. to ``2 u`` relative; (iii) nothing underflows (the smallest product of a test case
is far above ``2^-126``: :func:`assert_no_underflow`).  Pad terms are exact zeros (``x + 0 = x``) and count nothing.

* ``P[n, v] = sum_k H32 W32``: one product and at most ``K - 1`` additions touch a term (the first addition, to the zero
  accumulator, is exact): ``K u``; budgeted ``(K + 1) u``.
* ``R = X32 * rcp(P)``: ``2 u`` for the reciprocal, ``u`` for the product: ``+ 3 u``, so R is good to ``(K + 4) u``.
* ``U[n, k] = sum_v R W32``: ``V u``, budgeted ``(V + 1) u``.  Pad features: ``R = 0 * rcp(P) = 0`` exactly, because the pad
  columns of W hold 1 and ``P = sum_k H32 > 0`` there.
* ``H' = H32 * U``: ``+ u``.  Sum: ``(K + V + 7) u`` budgeted, and

      E_H = (K + V + 8) u

  with one more ``u`` for everything of second order.  The clip is exact (a comparison and a select).
* ``G[k, v] = sum_n H32 R``: R carries ``(K + 4) u``; a wave adds the ``16 T_w`` samples of its ``T_w`` tiles in fp32: one
  product and at most ``16 T_w - 1`` additions, budgeted ``(16 T_w + 1) u``.  The sums across the four waves of a workgroup and
  across workgroups are fp64.  ``T_w = ceil(ntiles / (4 grid))``, ``grid = min(compute units, ceil(ntiles / 4))``:
  wave ``w`` of workgroup ``b`` takes the tiles ``4 b + w + 4 grid j``.  So G is good to ``(K + 16 T_w + 5) u``.
* ``W' = W G / sum_v (W G)``: numerator and denominator each carry G's error (the denominator is again a sum of non-negative
  terms), the quotient twice that; the fp64 tail adds about ``(V + 4) 2^-53 < 1e-6 u``:

      E_W = 2 (K + 16 T_w + 8) u

  where ``2 (K + 16 T_w + 5) u`` is the derived part and ``6 u`` slack for second order and the fp64 tail.

An entry whose exact value before the clip lies within the bound of EPSILON may legitimately come back either as EPSILON or
as its value; both satisfy ``|dev - exact| <= bound * exact``.  Below ``EPSILON (1 - bound)`` it must be exactly EPSILON.
"""

from __future__ import annotations

import numpy as np

from oracle import klnmf_oracle as orc

EPS = orc.EPSILON  # 2^-23: exactly representable in fp32, so float32(EPSILON) == EPSILON
U32 = 2.0**-24
VMAX = 96
LD = np.longdouble
F32 = np.float32
AMBIGUOUS_SHARE = 1e-3


def tiles_per_wave(N: int, cus: int) -> int:
    """``T_w``: the most tiles one wave of ``fused_f32_kernel`` sums in fp32 (``salnmf_create``: grid)."""
    ntiles = (N + 15) // 16
    grid = min(cus, (ntiles + 3) // 4)
    return -(-ntiles // (4 * grid))


def bound_H(K: int, V: int) -> float:
    return (K + V + 8) * U32


def bound_W(K: int, T_w: int = 1) -> float:
    return 2 * (K + 16 * T_w + 8) * U32


def rounded(a) -> np.ndarray:
    """float64 image of the fp32 rounding of ``a``."""
    with np.errstate(over="ignore"):
        return np.asarray(a, dtype=np.float64).astype(F32).astype(np.float64)


def assert_no_underflow(X, W, H):
    """Assumption (iii) of the bound: the smallest product the step can form stays a normal fp32 number."""
    X, W, H = (rounded(a) for a in (X, W, H))
    tiny = float(np.finfo(F32).tiny) * 2.0**24
    pos = lambda a: float(np.min(a[a > 0])) if (a > 0).any() else 1.0
    P = H @ W
    r = pos(X) / float(np.nanmax(P))
    assert pos(H) * pos(W) > tiny and r * pos(W) > tiny and r * pos(H) > tiny


def _tail(W, G, n_given):
    """``clip(normalise(W * G))`` with the given rows restored (``_utils_klnmf.py:333-341``), before and after the clip."""
    K = W.shape[0]
    if n_given >= K:
        return W.copy(), W.copy()  # untouched, not even clipped (:330-331)
    Wp = W * G
    Wp = Wp / Wp.sum(axis=1, keepdims=True)
    Wp[:n_given] = W[:n_given]
    return Wp, np.clip(Wp, EPS, None)


def exact_step(X, W, H, n_given=0):
    """The fast mode's step without its rounding errors: ``(H', W', H_pre, W_pre)`` as float64 arrays."""
    X32, H32, W32 = (rounded(a).astype(LD) for a in (X, H, W))
    with np.errstate(divide="ignore", invalid="ignore", over="ignore"):
        R = X32 / (H32 @ W32)
        Hp = H32 * (R @ W32.T)
        Wp, Wn = _tail(np.asarray(W, dtype=np.float64).astype(LD), H32.T @ R, n_given)
    Hn = np.maximum(Hp, LD(EPS))  # (a NaN stays a NaN)
    return tuple(np.asarray(a, dtype=np.float64) for a in (Hn, Wn, Hp, Wp))


def _sum4(terms):
    """fp32 sum of up to four arrays as one k-step of the MFMA might form it: pairwise."""
    while len(terms) > 1:
        terms = [terms[i] + terms[i + 1] if i + 1 < len(terms) else terms[i] for i in range(0, len(terms), 2)]
    return terms[0]


def _dot32(A, B, order, skip=()):
    """``A (n, m) @ B (m, p)`` in float32, summed over ``m`` sequentially (order 0) or in steps of four (order 1)."""
    acc = np.zeros((A.shape[0], B.shape[1]), dtype=F32)
    idx = [j for j in range(A.shape[1]) if j not in skip]
    if order == 0:
        for j in idx:
            acc = acc + A[:, j : j + 1] * B[j : j + 1, :]
        return acc
    for s in range(0, A.shape[1], 4):
        terms = [A[:, j : j + 1] * B[j : j + 1, :] for j in range(s, min(s + 4, A.shape[1])) if j not in skip]
        if terms:
            acc = acc + _sum4(terms)
    return acc


def replica_step(X, W, H, n_given=0, order=0, cus=256, mutate=None, stale_H=None):
    """The step in float32 NumPy, as the kernel lays it out: ``(H', W')`` as float64 arrays.

    ``order`` 0 sums signatures, features and samples one after the other; ``order`` 1 in groups of four, pairwise
    inside a group, as the k-steps of the MFMA group them (samples ``{r, 4 + r, 8 + r, 12 + r}`` of a tile in the G
    phase).  G is summed in float32 per wave (its ``T_w`` tiles, in the kernel's order) and in float64 across waves.

    ``mutate`` plants one bug (``tests/test_f32_ref_host.py``): ``"u_last_feature"`` leaves feature ``V - 1`` out of U,
    ``"g_sample15"`` sample 15 of every tile out of G, ``"stale"`` reads ``stale_H`` instead of H, ``"floor0"`` writes the
    floor as 0, ``"wpad0"`` keeps 0 instead of 1 in the pad columns of W, ``"p_drop"`` leaves signature ``4 (K // 4)`` out of P.
    """
    X, W, H = (np.asarray(a, dtype=np.float64) for a in (X, W, H))
    N, V = X.shape
    K = W.shape[0]
    ntiles = (N + 15) // 16
    Np = 16 * ntiles
    X32 = np.zeros((Np, VMAX), dtype=F32)
    with np.errstate(over="ignore"):
        X32[:N, :V] = X.astype(F32)
        H32 = np.ones((Np, K), dtype=F32)  # pad rows 1 (salnmf_upload_H)
        H32[:N] = (stale_H if mutate == "stale" else H).astype(F32)
        W32 = np.full((K, VMAX), 0.0 if mutate == "wpad0" else 1.0, dtype=F32)
        W32[:, :V] = W.astype(F32)
    with np.errstate(divide="ignore", invalid="ignore", over="ignore"):
        drop = (4 * (K // 4),) if mutate == "p_drop" and K % 4 else ()
        P = _dot32(H32, W32, order, skip=drop)
        R = X32 * (F32(1.0) / P)
        U = _dot32(R, np.ascontiguousarray(W32.T), order, skip=(V - 1,) if mutate == "u_last_feature" else ())
        Hp = H32 * U
        floor = F32(0.0) if mutate == "floor0" else F32(EPS)
        Hn = np.where(Hp < F32(EPS), floor, Hp)  # a NaN stays a NaN
        # G: wave g = tile mod (4 grid) adds its tiles' samples in fp32
        grid = min(cus, (ntiles + 3) // 4)
        nw, T_w = 4 * grid, -(-ntiles // (4 * grid))
        Hw = np.zeros((T_w * nw * 16, K), dtype=F32)
        Rw = np.zeros((T_w * nw * 16, VMAX), dtype=F32)
        Hw[:Np], Rw[:Np] = H32, R
        Hw, Rw = Hw.reshape(T_w, nw, 16, K), Rw.reshape(T_w, nw, 16, VMAX)
        acc = np.zeros((nw, K, VMAX), dtype=F32)
        last = 15 if mutate == "g_sample15" else 16
        for t in range(T_w):
            term = lambda i: Hw[t, :, i, :, None] * Rw[t, :, i, None, :]
            if order == 0:
                for i in range(last):
                    acc = acc + term(i)
            else:
                for r in range(4):
                    acc = acc + _sum4([term(i) for i in (r, 4 + r, 8 + r, 12 + r) if i < last])
        G = acc.astype(np.float64).sum(axis=0)[:, :V]
        _, Wn = _tail(W, G, n_given)
    return Hn[:N].astype(np.float64), Wn


def ambiguous_share(pre, bound) -> float:
    """The share of entries whose exact value before the clip lies within ``bound`` of EPSILON."""
    pre = np.asarray(pre, dtype=np.float64)
    return float(np.mean(np.abs(pre - EPS) <= bound * EPS)) if pre.size else 0.0


def check(dev, exact, pre, bound, what=""):
    """``dev`` against :func:`exact_step`'s value ``exact`` (clipped) and ``pre`` (before the clip), entry by entry.

    (a) the NaN and the inf masks are identical; (b) ``|dev - exact| <= bound * exact`` for every finite entry; (c) where
    ``pre < EPSILON (1 - bound)``, ``dev`` is exactly EPSILON; (d) entries with ``pre`` within ``bound`` of EPSILON may be
    either value (both pass (b)), and their share is at most ``AMBIGUOUS_SHARE``.  Returns the largest error / bound."""
    dev, exact, pre = (np.asarray(a, dtype=np.float64) for a in (dev, exact, pre))
    assert dev.shape == exact.shape == pre.shape, (what, dev.shape, exact.shape)
    assert np.array_equal(np.isnan(dev), np.isnan(exact)), f"{what}: NaN masks differ ({np.isnan(dev).sum()} vs {np.isnan(exact).sum()})"
    assert np.array_equal(np.isinf(dev), np.isinf(exact)), f"{what}: inf masks differ ({np.isinf(dev).sum()} vs {np.isinf(exact).sum()})"
    assert np.array_equal(dev[np.isinf(dev)], exact[np.isinf(exact)]), f"{what}: inf signs differ"
    fin = np.isfinite(exact)
    ratio = np.zeros(exact.shape)
    ratio[fin] = np.abs(dev[fin] - exact[fin]) / (bound * exact[fin])
    worst = float(ratio.max()) if ratio.size else 0.0
    if worst > 1.0:
        i = np.unravel_index(int(np.argmax(ratio)), ratio.shape)
        raise AssertionError(f"{what}: error {worst:.3f} x the bound {bound:.3e} at {i}: dev {dev[i]!r} exact {exact[i]!r} (before the clip {pre[i]!r})")
    below = fin & (pre < EPS * (1.0 - bound))
    off = below & (dev != EPS)
    assert not off.any(), f"{what}: {int(off.sum())} of {int(below.sum())} entries below the floor are not exactly EPSILON, e.g. {dev[off][:4]!r}"
    share = ambiguous_share(pre[fin], bound)
    assert share <= AMBIGUOUS_SHARE, f"{what}: {share:.2e} of the entries lie within the bound of EPSILON"
    return worst


# ------------------------------------------------------------------ the cases of the one-step tests (host and GPU)

GEOMETRY_K = [1, 4, 5, 8, 9, 16, 17, 32, 33, 40, 41, 52, 53, 64]  # both ends of every KS in {1, 2, 4, 8, 10, 13, 16}
SHAPES = [(39, 96), (39, 83), (16, 7), (1, 96)]  # three tiles with a ragged last one, V < 96, one full tile, one sample
FLOOR_QUARTER = 0.25


def one_step_cases():
    """``(K, N, V, n_given)`` of the one-step tests."""
    out = []
    for K in GEOMETRY_K:
        for N, V in SHAPES:
            for g in sorted({0, min(2, K - 1)}):
                out.append((K, N, V, g))
    return out


def floor_share(a) -> float:
    return float(np.mean(np.asarray(a) == EPS))


def uses_floor_state(K, N, V) -> bool:
    """Where a quarter of H can sit at the floor: at least four signatures (a sample has one to ``K // 4`` active ones, so
    with fewer than four none can be spared) and more than one sample (the generator's single all-zero sample has no
    exposure structure at all)."""
    return K >= 4 and N > 1


_STATES = {}


def case_state(K, N, V, g, steps=80):
    """Inputs of one case, computed once and shared (read-only): a floor state of the oracle where the shape allows a
    quarter of H at the floor -- asserted -- and the dense synthetic problem otherwise.  (Eighty steps of the oracle:
    after the forty of ``test_gpu_floor.py`` two of the small shapes here have 19 % and 22 % of H at the floor.)"""
    key = (K, N, V, g)
    if key not in _STATES:
        seed = 1000 * K + 10 * N + V + g
        if uses_floor_state(K, N, V):
            X, W, H = orc.floor_state(V, N, K, seed, steps=steps, n_given=g, active=(1, max(1, min(4, K // 4))))
            assert floor_share(H) >= FLOOR_QUARTER, f"input H of {key}: only {floor_share(H):.2f} at the floor"
        else:
            X, W, H = orc.synthetic_problem(V, N, K, seed)
        for a in (X, W, H):
            a.setflags(write=False)
        _STATES[key] = (X, W, H)
    return _STATES[key]


_EXACT = {}


def case_exact(K, N, V, g):
    """:func:`exact_step` of :func:`case_state`, computed once."""
    key = (K, N, V, g)
    if key not in _EXACT:
        X, W, H = case_state(*key)
        _EXACT[key] = exact_step(X, W, H, g)
    return _EXACT[key]


MI355X_CUS = 256
MANY_TILES_K = [8, 36]
CHAINED_K = [5, 36, 64]


def many_tiles_samples(cus: int) -> int:
    """More tiles than one round of the grid's waves, a ragged last tile: ``T_w = 2``."""
    return 16 * (4 * cus + 5) + 3


def many_tiles_state(K, cus):
    return case_state(K, many_tiles_samples(cus), VMAX, 0, steps=30)


BIG_COUNTS = (2.0**24 + 1, 3e7, 1e9)


def big_counts_state():
    """A dense catalogue with a few entries beyond fp32's integers (2^24 + 1 rounds to 2^24: a tie, to even), W and H
    already fp32 numbers so that X is the only input the shadow copies round: ``(X, W, H)``, K = 12, N = 39."""
    key = "big"
    if key not in _STATES:
        V, N, K = 96, 39, 12
        X, W, _ = orc.synthetic_problem(V, N, K, seed=7)
        X[0, 3], X[5, 10], X[17, 95], X[38, 0], X[38, 50] = BIG_COUNTS[0], BIG_COUNTS[1], BIG_COUNTS[2], BIG_COUNTS[0], BIG_COUNTS[2]
        H = X.sum(axis=1)[:, None] * np.random.default_rng(7).dirichlet(np.ones(K), size=N)
        W, H = rounded(W), rounded(H)
        assert (rounded(X) != X).any()
        for a in (X, W, H):
            a.setflags(write=False)
        _STATES[key] = (X, W, H)
    return _STATES[key]
