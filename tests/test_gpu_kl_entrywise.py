"""The KL objectives on the device against an extended-precision reference (``tests/_kl_ref.py``), sample by sample.

(A) Logarithm probes through the real kernels, one entry at a time.  ``Engine(N, V, 1)`` with W made of powers of two:
    ``P[n, v] = H[n] W[v]`` is exact.  A probe sample has one non-zero count x at one feature v* (W[v*] = 1, H[n] = p); its
    other features have x = 0 and contribute their p only (W = 2^-60 there; W = 1 where p 2^-60 would not be a normal
    number -- such p are below 2^-900 and negligible against x |log p|).  The probes are spread over feature positions that
    cover all 16 lane columns c16 and all six feature tiles vt; the four q rows come with the sample index.
    Mode 1 (``log_ratio``): ``samplewise_kl()`` returns the sample.  Mode 0 (``log_pos``): ``objective()`` under one-hot
    sample weights -- ``tile_kl<true>`` multiplies each finite lane sum by its sample's weight, an exact 0 or 1, before any
    sum over lanes (salnmf_kernels.h: ``if (ROWS) acc *= wv[r]``), and the sums that follow add exact zeros, so the result
    is sample n's 16 lane values summed.
    Shapes: all tiles full at V = 96 (fast branch); N = 17 (the 17th sample sits in a ragged tile: masked branch);
    V = 83 and V = 7 (masked by features); every 16th sample with H = 3e-308 (P subnormal: its tile, i.e. every tile, takes
    the library branch); V = 97 and V = 192 (feature blocks, the last block of V = 97 one feature wide).
(B) Whole samples in both modes against ``kl_rows`` within ``SLACK x`` the recorded yardstick of the mode, and the weighted
    objective under random weights.
(C) The objective folded into the step (``kl_step_objective`` / ``objective_read``), including a cooperative leftover tile,
    and the KL part of the value an MvNMF step accepts (``tile_kl<false>`` with all six logarithms side by side).
(D) ``KLNMFSweep`` held-out scores per sample and per member in the mode 1 unit.

Every assertion names the sample, its unit, the ratio and the branch it was meant to reach; run with ``-s`` for the measured
ratios (recorded in DESIGN.md, "Accuracy of the KL objectives")."""

import functools

import mpmath as mp
import numpy as np
import pytest

import _kl_ref as R
from salamander_amd.engine import Engine

pytestmark = pytest.mark.gpu

EPS = R.EPS64
SUBNORMAL_H = 3e-308


# ------------------------------------------------------------------------------------------------------ (A) the probes
@functools.lru_cache(maxsize=None)
def _probes():
    """[(x, p, mode, label)]: mode 0 probes of log_pos (the host test's set with 256 of its random arguments) and mode 1
    probes of log_ratio (the host test's set and the operands just outside log_operand_ok), with the exact values of
    ``x log x - x - x log p + p`` (mode 0) / ``x log(x / p) - x + p`` (mode 1) and of log p / log(x / p)."""
    out = []
    for t, (p, label) in enumerate(R.log_pos_probes(256)):
        lg = abs(float(np.log(p)))
        # x |log p| ~ p where p is large: the log term stays visible.  Near the top of the range x = p 2^-16 instead: x log x ~ p
        # would leave no room for the sample's value under another probe position's W (0 x inf under a one-hot weight)
        x = float(1000 + t % 977) if p <= 1e3 else (p / max(lg, 1.0) if p <= 2.0**1000 else p * 2.0**-16)
        out.append((x, p, 0, label))
    for x, p, label in R.log_ratio_probes():
        out.append((x, p, 1, label))
    for x, p, label in R.log_ratio_outside():
        out.append((x, p, 2, label))  # mode 1 through the per-entry library fallback
    exact = []
    with mp.workdps(R.DPS):
        for x, p, mode, _ in out:
            xm, pm = mp.mpf(x), mp.mpf(p)
            if mode == 0:
                exact.append((xm * mp.log(xm) - xm - xm * mp.log(pm) + pm, mp.log(pm)))
            else:
                exact.append((xm * mp.log(xm / pm) - xm + pm, mp.log(xm / pm)))
    return out, exact


@pytest.fixture(scope="module", autouse=True)
def _release():
    yield
    _probes.cache_clear()
    _whole.cache_clear()


def _positions(V):
    """probe features: every lane column c16 = v mod 16, every feature tile vt = v // 16 that V has, every feature block"""
    if V >= 96:
        pos = [16 * (c % 6) + c for c in range(16)]
        if V > 96:
            pos += [96 + 16 * (c % ((V - 96 + 15) // 16)) + c for c in range(16) if 96 + 16 * (c % ((V - 96 + 15) // 16)) + c < V] + [V - 1]
        return sorted(set(pos))
    nt = (V + 15) // 16
    return sorted({v for c in range(16) for v in [16 * (c % nt) + c] if v < V} | {V - 1})


def _run_probes(tag, V, idx, n_engine=None, subnormal=False, fixed_position=None, K=1, lead=0, quiet=False):
    """The probes ``idx`` (indices into ``_probes()``) on one engine of V features: every probe asserted, the worst ratios
    (error / bound) per mode returned with their labels.  ``K`` > 1: K identical rows of W and one active signature per
    sample (H zero elsewhere), cycling through the signatures: P is a K-term sum whose value is still exact.  ``lead``: that
    many filler samples first (a full tile in front of a ragged one)."""
    probes, exact = _probes()
    pos = _positions(V) if fixed_position is None else [fixed_position]
    rows, sub_rows = [-1] * lead, []  # sample -> probe index, -1 (benign filler: x = 0, H = 1) or None (subnormal extra)
    for j, t in enumerate(idx):
        if subnormal and len(rows) % 16 == 15:
            sub_rows.append(len(rows))
            rows.append(None)
        rows.append(t)
    if subnormal:
        while len(rows) % 16 != 15:
            rows.append(-1)  # benign filler
        sub_rows.append(len(rows))
        rows.append(None)
    N = n_engine if n_engine is not None else len(rows)
    while len(rows) < N:
        rows.append(-1)
    assert len(rows) == N
    vstar = np.array([pos[n % len(pos)] for n in range(N)])
    X = np.zeros((N, V))
    Hbase = np.ones(N)
    member = {}
    for n, t in enumerate(rows):
        if t is None:
            X[n, vstar[n]], Hbase[n] = 1.0, SUBNORMAL_H
        elif t >= 0:
            x, p, mode, _ = probes[t]
            X[n, vstar[n]] = x
            member.setdefault((int(vstar[n]), p < 2.0**-900), []).append(n)
    for n in sub_rows:  # checked with every group of their position
        for key in list(member):
            if key[0] == vstar[n]:
                member[key].append(n)
    e = Engine(N, V, K)
    active = np.arange(N) % K
    e.upload_X(X)
    worst = {0: (0.0, ""), 1: (0.0, "")}
    for (v, tiny), ns in sorted(member.items()):
        wo = 1.0 if tiny else 2.0**-60
        W = np.full((1, V), wo)
        W[0, v] = 1.0
        H = Hbase.copy()
        if tiny:  # (W = 1 everywhere: 3e-308 itself is a normal number, a quarter of it is not)
            H[H == SUBNORMAL_H] = SUBNORMAL_H / 4
        for n in ns:
            if rows[n] is not None:
                H[n] = probes[rows[n]][1]
        e.upload_W(np.tile(W, (K, 1)))
        HK = np.zeros((N, K))
        HK[np.arange(N), active] = H
        e.upload_H(HK)
        e.set_weights(None, None)
        sk = e.samplewise_kl()
        for n in ns:
            if rows[n] is None:
                x, p, mode, label = 1.0, float(H[n]), 3, "subnormal-P sample"
                with mp.workdps(R.DPS):
                    lp = mp.log(mp.mpf(p))
                    base = mp.mpf(x) * mp.log(mp.mpf(x)) - x - x * lp + mp.mpf(p)
                    lr = mp.log(mp.mpf(x) / mp.mpf(p))
            else:
                x, p, mode, label = probes[rows[n]]
                base, lr = exact[rows[n]]
                lp = lr
            with mp.workdps(R.DPS):
                others = mp.fsum(mp.mpf(float(H[n] * W[0, u])) for u in range(V) if u != v)  # (float64 products, as the device forms them: exact or subnormal-rounded)
                want = base + others
            # 4 x 2^-52 x (sum_v p [+ the unit's K-term product term (K + 1) |p - x|, as the issue states it]), scaled term by term: the
            # sum itself overflows for the probes at exponent 1023
            S = 4 * 2.0**-52
            tail_p = S * float(others) + S * p + (0.0 if K == 1 else (K + 1) * (S * abs(p - x)))
            where = f"{tag} sample {n} (q={n % 4}, c16={v % 16}, vt={v // 16 % 6}, block {v // 96}) '{label}' x={x!r} p={p!r}"
            if mode in (1, 2, 3):
                got = float(sk[n])
                b_log = R.log_ratio_bound(x, p, lr) if mode == 1 else 2.0**-52 * (abs(float(lr)) + 1.0)  # library log of the rounded quotient
                bound = x * b_log + S * x + tail_p
                err = abs(float(mp.mpf(got) - want))
                assert np.isfinite(bound), where
                r = err / bound
                if r > worst[1][0]:
                    worst[1] = (r, label)
                assert r <= 1.0, f"mode 1, {where}: got {got!r}, exact {float(want)!r}, error {err:.3e} = {r:.2f} x its bound {bound:.3e}"
            if mode in (0, 3):
                w = np.zeros(N)
                w[n] = 1.0
                e.set_weights(w, None)
                got = e.objective()
                al = abs(float(lp))
                b_log = R.LOG_POS_REL * max(al, 0.5) if mode == 0 and not subnormal else 2.0**-52 * max(al, 0.5)
                with mp.workdps(R.DPS):
                    xlx = abs(float(mp.mpf(x) * mp.log(mp.mpf(x)) - x))
                bound = x * b_log + S * xlx + S * (x * al) + tail_p
                assert np.isfinite(bound), where
                err = abs(float(mp.mpf(got) - want))
                r = err / bound
                if r > worst[0][0]:
                    worst[0] = (r, label)
                assert r <= 1.0, f"mode 0, {where}: got {got!r}, exact {float(want)!r}, error {err:.3e} = {r:.2f} x its bound {bound:.3e}"
    e.close()
    for m in (0, 1) if not quiet else ():
        print(f"\n[kl-entrywise] {tag}: mode {m} worst {worst[m][0]:.3f} of its bound at '{worst[m][1]}'")
    return worst


def _all_idx():
    return list(range(len(_probes()[0])))


@pytest.mark.parametrize("V,branch", [(96, "fast"), (83, "masked by features"), (7, "masked by features"), (97, "feature blocks, last block 1 wide"),
                                      (192, "feature blocks")])
def test_logarithm_probes_full_tiles(V, branch):
    idx = _all_idx()
    idx += [idx[-1]] * (-len(idx) % 16)  # all tiles full
    _run_probes(f"V={V} N={len(idx)} ({branch} branch)", V, idx)


def test_logarithm_probes_through_the_signature_chunk_chain():
    """K = 65: two chunks (64 + 1 signatures), the second launch continues from the first one's P (PIN) and evaluates the
    divergence.  Every probe has one active signature, cycling through all 65, so the probed product arrives through either
    chunk; the K-term sum is exact and the bound carries the (K + 1) |p - x| term all the same."""
    idx = _all_idx()
    idx += [idx[-1]] * (-len(idx) % 16)
    _run_probes(f"V=96 N={len(idx)} K=65 (signature chunks, PIN chain)", 96, idx, K=65)


def test_logarithm_probes_ragged_tile():
    """Every probe in a ragged tile: engines of N = 16 + r samples, a full tile of fillers (fast branch) and the probes in
    the r rows of the second, ragged tile (masked branch); r = 15 mostly, every fifth engine another r in 1 .. 14, N = 17
    among them.  Only the ragged tile's samples are asserted and reported."""
    idx = _all_idx()
    worst, g, at = {0: (0.0, ""), 1: (0.0, "")}, 0, 0
    positions = _positions(96)
    while at < len(idx):
        r = 15 if g % 5 else 1 + (g // 5) % 14
        w = _run_probes(f"V=96 N={16 + r} engine {g} (masked branch, ragged tile of {r})", 96, idx[at : at + r], n_engine=16 + min(r, len(idx) - at),
                        fixed_position=positions[g % len(positions)], lead=16, quiet=True)
        worst = {m: max(worst[m], w[m]) for m in (0, 1)}
        at, g = at + r, g + 1
    for m in (0, 1):
        print(f"\n[kl-entrywise] ragged tiles ({g} engines, masked branch): mode {m} worst {worst[m][0]:.3f} of its bound at '{worst[m][1]}'")


def test_logarithm_probes_beside_a_subnormal_sample():
    """Every 16th sample has H = 3e-308 (a quarter of that where W = 1 everywhere, i.e. beside the probes with p < 2^-900):
    its P are subnormal (or zero where x = 0), finite, so every tile takes the library branch.  The probes that share the tiles keep their bounds (mode 0 with the library logarithm's ulp in place of
    log_pos's bound where it is larger), the subnormal samples' own values are held to the library log's error."""
    _run_probes("V=96 (library branch: one subnormal-P sample per tile)", 96, _all_idx(), subnormal=True, fixed_position=37)


# ------------------------------------------------------------------------------------------------- (B) whole samples
@functools.lru_cache(maxsize=None)
def _whole(kind, V, N, K):
    X, W, H, exact_p = R.whole_state(kind, V, N, K)
    ref = {}
    for mode in (0, 1):
        worst, want, u = R.oracle_ratio(X, W, H, mode, exact_p)
        assert worst <= R.ORACLE_RATIO[mode], f"{kind} V={V} N={N} K={K} mode {mode}: the float64 restatement reaches {worst:.3f} on the CPU"
        allow = R.SLACK * R.ORACLE_RATIO[mode] * EPS * u
        ref[mode] = (want, u, allow)
    return X, W, H, ref


def _engine(X, W, H):
    e = Engine(X.shape[0], X.shape[1], W.shape[0])
    e.upload_X(X), e.upload_W(W), e.upload_H(H)
    return e


def _branch(kind, V, N):
    if kind == "subnormal":
        return "library branch beside normal samples"
    return "fast branch, ragged last tile masked" if V == 96 and N % 16 else ("fast branch" if V == 96 else "masked / blocked branch")


@pytest.mark.parametrize("V,N,K", R.WHOLE_SHAPES)
def test_whole_samples_both_modes(V, N, K):
    rng = np.random.default_rng(V + N + K)
    for kind in ("catalogue", "near", "exact", "floor", "subnormal"):
        if (kind, V, N, K) not in R.whole_cases():
            continue
        X, W, H, ref = _whole(kind, V, N, K)
        tag = f"{kind} V={V} N={N} K={K} ({_branch(kind, V, N)})"
        e = _engine(X, W, H)
        got = {1: e.samplewise_kl(), 0: np.empty(N)}
        for n in range(N):
            w = np.zeros(N)
            w[n] = 1.0
            e.set_weights(w, None)
            got[0][n] = e.objective()
        wts = rng.uniform(0.1, 3.0, N)
        e.set_weights(wts, None)
        weighted = e.objective()
        e.close()
        for mode in (0, 1):
            want, u, allow = ref[mode]
            err = np.abs(got[mode].astype(R.L) - want).astype(np.float64)
            n = int(np.argmax(err / allow))
            print(f"\n[kl-entrywise] {tag} mode {mode}: worst {float((err / (EPS * u)).max()):.4f} x 2^-53 u (allowed {R.SLACK * R.ORACLE_RATIO[mode]:.3f})")
            assert np.isfinite(got[mode]).all(), tag
            assert err[n] <= allow[n], (f"{tag} mode {mode}: sample {n} got {got[mode][n]!r}, exact {float(want[n])!r}, unit {u[n]:.3e}, ratio "
                                        f"{err[n] / (EPS * u[n]):.3f} against {R.SLACK * R.ORACLE_RATIO[mode]:.3f}; {int((err > allow).sum())} samples over")
        want, u, allow = ref[0]
        werr = abs(float(R.L(weighted) - (wts.astype(R.L) * want).sum()))
        assert werr <= float((wts * allow).sum()), f"{tag}: weighted objective off by {werr:.3e}, allowed {float((wts * allow).sum()):.3e}"


# ------------------------------------------------------------------------------- (C) the objective folded into the step
# K -> (KS, KTM, KR) of the fused pass (test_gpu_floor.py: GEOMETRY_K): K = 8 has KR = 0, tile_kl<false, 3>; K = 19 has
# KR = 3, tile_kl<false, 2> (salnmf_fused_kernel.h: MB = KR >= 3 ? 2 : 3).  The small-cohort kernel is switched off, or
# kl_step_objective would take a forward pass for these sizes.
def _folded(X, W, H):
    e = _engine(X, W, H)
    e.set_small_cohort_tiles(0)
    e.kl_step_objective(0, 1)
    v = float(e.objective_read(0, 1)[0])
    e.close()
    e = _engine(X, W, H)
    o = e.objective()
    e.close()
    return v, o


def _check_total(tag, X, W, H, exact_p=False):
    worst, want, u = R.oracle_ratio(X, W, H, 0, exact_p)
    assert worst <= R.ORACLE_RATIO[0], f"{tag}: the float64 restatement reaches {worst:.3f} on the CPU"
    total, allow = want.sum(), float(R.SLACK * R.ORACLE_RATIO[0] * EPS * u.sum())
    folded, plain = _folded(X, W, H)
    ef, ep = abs(float(R.L(folded) - total)), abs(float(R.L(plain) - total))
    print(f"\n[kl-entrywise] {tag}: folded {ef / (EPS * u.sum()):.4f}, objective() {ep / (EPS * u.sum()):.4f} x 2^-53 sum u (allowed {R.SLACK * R.ORACLE_RATIO[0]:.3f})")
    assert ef <= allow, f"{tag}: folded objective {folded!r} against {float(total)!r}: off by {ef:.3e}, allowed {allow:.3e}"
    assert ep <= allow, f"{tag}: objective() {plain!r} against {float(total)!r}: off by {ep:.3e}, allowed {allow:.3e}"
    assert abs(folded - plain) <= 2 * allow, (tag, folded, plain)


@pytest.mark.parametrize("kind", ["near", "catalogue"])
@pytest.mark.parametrize("K,V", [(8, 96), (19, 96), (8, 83), (19, 83)])
def test_objective_folded_into_the_step(K, V, kind):
    N = 16 * 5 + 7
    X, W, H, exact_p = R.whole_state(kind, V, N, K)
    _check_total(f"folded {kind} V={V} N={N} K={K} (tile_kl<false, {2 if K == 19 else 3}>)", X, W, H, exact_p)


@pytest.mark.parametrize("V", [96, 83])
def test_objective_folded_with_a_cooperative_leftover_tile(V):
    """16 400 samples are 1 025 tiles, one more than a round of the grid's waves (test_gpu_floor.py): the leftover tile runs
    as a cooperative tile, whose KL terms are a masked copy of tile_kl (salnmf_fused_kernel.h)."""
    N, K = 16400, 50
    X, W, H, exact_p = R.whole_state("catalogue", V, N, K)
    _check_total(f"cooperative tile V={V} N={N} K={K}", X, W, H, exact_p)


@pytest.mark.parametrize("queued", [True, False])
@pytest.mark.parametrize("K,V", [(8, 96), (19, 83)])
def test_kl_part_of_the_accepted_mvnmf_objective(K, V, queued):
    """The third instantiation of the folded call, ``tile_kl<false>`` with MB = VT (salnmf_fused_kernel.h, the
    ``DO_STATS && !JKL`` branch): the update_H pass that evaluates an MvNMF trial while it already runs the next step's
    first half -- the update_H half of the queued joint pass, the speculative pass of the classic form.  Those passes run
    only where another step follows, so the call is ``mv_step_objective(1, ..., more_follows=True)``: its value is then
    that pass's KL sum of (W_trial, clip(H colsum)) + lam log det -- provided the first trial was accepted (gamma comes
    back as min(1, 1.2 gamma); a rejected trial is re-scored by a forward pass), which is asserted.  The downloads step the
    engine back to the accepted state.  With the log det taken from the reference (``_mv_ref``), the KL part is held to the
    sum of the samples' allowances.  (The numerator half's ``klacc_b`` is the same inlined call on the next state; it only
    ever feeds the next step's f0 and no API returns it.)"""
    import _mv_ref as M

    N, lam, delta = 16 * 5 + 7, 1.0, 1.0
    X, W, H, _ = R.whole_state("catalogue", V, N, K)
    e = _engine(X, W, H)
    e.set_mv_queued(queued)
    gamma, f = e.mv_step_objective(1, 0, lam, delta, 1.0, more_follows=True)
    assert gamma == 1.0, f"the first trial was not accepted (gamma {gamma}): the value read is not the speculative pass's"
    W1, H1 = e.download_W(), e.download_H()
    e.close()
    worst, want, u = R.oracle_ratio(X, W1, H1, 0)
    assert worst <= R.ORACLE_RATIO[0], f"the float64 restatement reaches {worst:.3f} on the CPU"
    ref = M.MvRef(W1, delta)
    allow = float(R.SLACK * R.ORACLE_RATIO[0] * EPS * u.sum()) + lam * M.C["logdet"] * EPS * ref.logdet_scale
    err = abs(float(R.L(f) - (want.sum() + R.L(lam * float(ref.logdet)))))
    print(f"\n[kl-entrywise] MvNMF accepted objective K={K} V={V} queued={queued}: {err / (EPS * u.sum()):.4f} x 2^-53 sum u (gamma {gamma})")
    assert err <= allow, f"K={K} V={V} queued={queued}: accepted objective {f!r} against {float(want.sum()) + lam * float(ref.logdet)!r}: off by {err:.3e}, allowed {allow:.3e}"


# ------------------------------------------------------------------------------------------------ (D) held-out scores
def test_sweep_heldout_scores_per_sample():
    """32 samples, K = 2 and 3, one split: ``obs["heldout_error"]`` per sample and ``heldout_errors_`` per member against
    ``kl_rows(max(test, EPSILON), W, max(c H, EPSILON))`` in the mode 1 unit."""
    import salamander_amd as sal

    rng = np.random.default_rng(11)
    Wt = rng.dirichlet(np.full(96, 0.2), size=3)
    X = rng.poisson(rng.dirichlet(np.full(3, 0.5), size=32) * 2000.0 @ Wt).astype(float)
    p = 0.5
    s = sal.models.KLNMFSweep([2, 3], seeds=[0], n_splits=1, train_fraction=p, split_seed=2024, init_method="random", min_iterations=20,
                              max_iterations=40, conv_test_freq=10)
    models = s.fit(sal.AnnData(X.copy()))
    assert len(models) == 2 and s.heldout_errors_.shape == (2, 1, 1)
    c = (1.0 - p) / p
    for i, m in enumerate(models):
        Xt = np.maximum(s.test_splits_[s.split_of_[i]], R.EPSILON)
        W = np.asarray(m.asignatures.X, dtype=np.float64)
        H = np.maximum(c * np.asarray(m.adata.obsm["exposures"], dtype=np.float64), R.EPSILON)
        worst, want, u = R.oracle_ratio(Xt, W, H, 1)
        assert worst <= R.ORACLE_RATIO[1], f"member {i}: the float64 restatement reaches {worst:.3f} on the CPU"
        allow = R.SLACK * R.ORACLE_RATIO[1] * EPS * u
        got = np.asarray(m.adata.obs["heldout_error"], dtype=np.float64)
        err = np.abs(got.astype(R.L) - want).astype(np.float64)
        n = int(np.argmax(err / allow))
        print(f"\n[kl-entrywise] held-out K={m.n_signatures}: worst {float((err / (EPS * u)).max()):.4f} x 2^-53 u1 (allowed {R.SLACK * R.ORACLE_RATIO[1]:.2f})")
        assert err[n] <= allow[n], (f"held-out K={m.n_signatures}: sample {n} got {got[n]!r}, exact {float(want[n])!r}, unit {u[n]:.3e}, ratio "
                                    f"{err[n] / (EPS * u[n]):.3f}")
        total = float(s.heldout_errors_.reshape(-1)[i])
        terr = abs(float(R.L(total) - want.sum()))
        # (the member's total is a host-side float64 sum of the 32 per-sample values: at most 32 roundings of the running sum)
        assert terr <= float(allow.sum()) + 32 * EPS * float(np.abs(want).sum()), (m.n_signatures, total, float(want.sum()))
