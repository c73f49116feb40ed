"""The pending exposure scale, through every reader of H (DESIGN.md "Pending exposure scale" is the list this file enforces).

After ``Engine.set_H_scale`` and after every accepted MvNMF trial the engine does not rewrite H: ``h_pending`` / ``cs`` say
that H is to be read as ``clip(H * cs, EPSILON)`` until a pass writes H in full.  Some readers apply the scale on the fly,
some materialise it first (``flush_H_scale``), some overwrite H and drop it.  A reader that forgets the scale, applies it
twice, flushes and leaves the flag set, or clears the flag without having written H gives a finite, plausible, wrong
factorisation.

**Twin engines.**  A holds ``(X, W, H)`` with the scale pending, B holds ``(X, W, Hs)`` with nothing pending, ``Hs`` the
materialised state in float64.  The pending state comes (i) from ``set_H_scale`` on a floor state with a scale that clips
whole columns and lifts floor entries (``tests/_scale_ref.py``; its conditions are asserted on the host by
``test_scale_ref_host.py``), and (ii) from one MvNMF step -- an accepted first trial and a backtracking one, queued and
classic; B's state is then downloaded from a second, identically driven engine (downloading from A would flush A).
Every reader is called on A with the scale freshly pending and on B, and

(a) both results are held to the entry point's existing reference on ``Hs`` at its existing tolerance
    (``test_gpu_floor``'s entry-wise constants, ``test_gpu_wide``'s bounds for the objectives and the CorrNMF pieces);
(b) A's result equals B's bit for bit: in the present code every reader either runs the same launch after a flush, or
    applies ``clip(h * cs[k], EPSILON)`` to the H tile it has just loaded and then does what it does without a scale --
    the same operations in the same order.  (The joint fused pass never applies a scale on the fly: ``launch_fused``
    flushes first, so the cooperative leftover tile runs with and without a pending scale and the numerator is summed in
    one order; ``test_cooperative_leftover_tile_with_a_scale_pending`` pins that.)
(c) the state afterwards is the right one: a reader that does not rewrite H gives the same bits when called again and
    ``download_H()`` is then ``Hs`` bit for bit; behind a reader that rewrites H the objective and the downloads agree
    with B's.
"""

import contextlib

import numpy as np
import pytest

import _scale_ref as S
import test_gpu_floor as tgf
from _floor import EPS
from conftest import rel_l2
from oracle import corrnmf_oracle as co
from oracle import klnmf_oracle as orc
from salamander_amd import Engine, _lib

pytestmark = pytest.mark.gpu

RT_STEP, RT_RUN, RT_MV_W, RT_MV_H, RT_F32, SKL_ABS = tgf.RT_STEP, tgf.RT_RUN, tgf.RT_MV_W, tgf.RT_MV_H, tgf.RT_F32, tgf.SKL_ABS
OBJ_RT = 1e-12   # test_gpu_wide.py::test_wide_functions_against_the_oracle: objective
SKL_RT = 1e-11   # ... samplewise_kl (with test_gpu_floor's absolute term per sample: all-EPSILON samples have a divergence near 0)
REC_L2 = 1e-14   # ... reconstruct
CORR_BOUND = 1e-12  # test_wide_corrnmf_dense_pieces_match_oracle
MV_OBJ_RT = 1e-11   # test_wide_mvnmf_steps_and_function_level_api_match_the_oracle: mv_objective, mv_logdet
MV_STEP_OBJ_RT = 1e-9  # ... the objective mv_step_objective returns

# ------------------------------------------------------------------ sources of a pending scale and paths

SCALE_SOURCES = [("scale",) + p for p in S.all_cases()]
MV_SOURCES = [("mv", name, queued) for name in S.MV_NARROW for queued in (True, False)]
SOURCES = SCALE_SOURCES + MV_SOURCES


def src_id(src):
    if src[0] == "scale":
        return "scale-" + S.case_id(src[1:])
    return f"mv-{src[1]}-{'queued' if src[2] else 'classic'}"


def src_shape(src):
    return src[1:4] if src[0] == "scale" else S.mv_case(src[1]).shape


PATHS = ("fused", "wkl", "wlh", "wboth")  # the plain fused path (small-cohort kernel off), and with per-sample weights
# the weighted instantiations are kernels of their own, one geometry class each suffices: KR == 0, KR != 0, feature blocks,
# and behind an MvNMF step
WEIGHTED_SOURCES = [("scale", 96, 39, 7, "both"), ("scale", 96, 215, 17, "both"), ("scale", 288, 215, 12, "both"), ("mv", "accepted", True)]


def small_ok(src):
    V, N, K = src_shape(src)
    return V <= 96 and K <= 16 and (N + 15) // 16 <= 64


def grid(sources, paths=PATHS, small=False):
    """``(source, path)`` pairs: every source on the plain path, ``WEIGHTED_SOURCES`` on the weighted ones; with ``small`` the
    small-cohort kernel where it takes the shape."""
    out = [(s, p) for s in sources for p in paths if p == "fused" or s in WEIGHTED_SOURCES]
    if small:
        out += [(s, "small") for s in sources if small_ok(s)]
    return out


def sp_id(sp):
    return f"{src_id(sp[0])}-{sp[1]}"


class Twins:
    """Engine A with a scale pending, engine B on the materialised state ``(W, Hs)``; ``arm()`` puts both back."""

    def __init__(self, src, path="fused", precision=None, queued=None):
        self.src, self.path = src, path
        self.queued = queued if queued is not None else (src[2] if src[0] == "mv" else None)
        if src[0] == "scale":
            c = S.case(*src[1:])
            self.X, self.W, self.H0, self.scale = c.X, c.W, c.H0, c.scale
            self.mv = None
        else:
            self.mv = S.mv_case(src[1])
            self.X, self.W0, self.H0 = self.mv.X, self.mv.W, self.mv.H
        self.N, self.V = self.X.shape
        self.K = self.H0.shape[1]
        rng = np.random.default_rng(self.N + self.K)
        self.wkl = rng.uniform(0.5, 2.0, self.N) if path in ("wkl", "wboth") else None
        self.wlh = rng.uniform(0.5, 5.0, self.N) if path in ("wlh", "wboth") else None
        self.engines = []
        self.precision = precision
        if self.mv is not None:
            # the materialised state of the MvNMF source: from a second, identically driven engine
            a2 = self._engine()
            self._mv_arm(a2)
            self.W, self.Hs = a2.download_W(), a2.download_H()
            a2.close()
            self.engines.remove(a2)
        else:
            self.Hs = S.materialise(self.H0, self.scale)
        self.A, self.B = self._engine(), self._engine()
        self.arm()

    def _engine(self):
        e = Engine(self.N, self.V, self.K)
        self.engines.append(e)
        e.set_small_cohort_tiles(64 if self.path == "small" else 0)
        if self.queued is not None:
            e.set_mv_queued(self.queued)
        e.upload_X(self.X)
        e.set_weights(self.wkl, self.wlh)
        if self.precision:
            e.set_precision(self.precision)
        return e

    def _mv_arm(self, e):
        m = self.mv
        e.upload_W(m.W), e.upload_H(m.H)
        gamma = e.mv_step(1, m.n_given, m.lam, m.delta, 1.0)
        # an accepted first trial returns min(1, 1.2 gamma) = 1, a backtracking one 1.2 * 0.8^j < 1 (as test_gpu_kl_entrywise.py)
        assert gamma == m.gamma and (gamma < 1.0) == m.backtracks, (gamma, m.gamma)

    def arm(self, which="AB"):
        if "A" in which:
            if self.mv is None:
                self.A.upload_W(self.W), self.A.upload_H(self.H0)
                self.A.set_H_scale(self.scale)
            else:
                self._mv_arm(self.A)
        if "B" in which:
            self.B.upload_W(self.W), self.B.upload_H(self.Hs)

    def both(self, fn):
        """``fn`` on A with the scale freshly pending, and on B."""
        self.arm()
        return fn(self.A), fn(self.B)

    def close(self):
        for e in self.engines:
            e.close()


@contextlib.contextmanager
def twins(src, path="fused", precision=None, queued=None):
    t = Twins(src, path, precision, queued)
    try:
        yield t
    finally:
        t.close()


def given_values(K):
    return sorted({0, min(2, K), K})


# ------------------------------------------------------------------ references (the oracle on the materialised state)


def oracle_steps(t, n, g, W=None, H=None):
    """``n`` joint steps of the oracle from ``(W, Hs)``: ``(W, H, W_pre, H_pre, H_allowance)`` of the last one."""
    W = t.W if W is None else W
    H = t.Hs if H is None else H
    for _ in range(n - 1):
        W, H = (a.T for a in orc.update_WH(t.X.T, W.T, H.T, t.wkl, t.wlh, g))
    return tgf.oracle_step(t.X, W, H, t.wkl, t.wlh, g)


def check_state(tag, t, e, want, rtol, g, n=1):
    """The engine's (W, H) against ``want = oracle_steps(...)``, entry by entry and exact at the floor."""
    Wn, Hn, Wp, Hp, allow = want
    margin = RT_F32 if rtol == RT_F32 else 1e-6
    if allow is not None and n > 1:
        allow = 8 * allow  # (test_gpu_floor.step_and_run: the allowance of a short run)
    tgf.check(f"{tag}/H", e.download_H(), Hn, rtol, pre=Hp, allowance=allow, margin=margin)
    if g < t.K:
        tgf.check(f"{tag}/W", e.download_W(), Wn, rtol, pre=Wp, margin=margin)
    else:
        assert np.array_equal(e.download_W(), t.W), f"{tag}: every signature given, W changed"


def check_objective(tag, got, X, W, H, wkl=None, wlh=None):
    want = orc.klnmf_objective(X.T, W.T, H.T, wkl, wlh)
    assert np.isclose(got, want, rtol=OBJ_RT, atol=0), f"{tag}: objective {got!r} vs {want!r} ({abs(got - want) / abs(want):.2e})"


def same_state(tag, t):
    """Behind a reader that rewrote H: A's and B's objectives and downloads are the same bits."""
    assert t.A.objective() == t.B.objective(), f"{tag}: objectives of the twins differ"
    assert np.array_equal(t.A.download_W(), t.B.download_W()), f"{tag}: W of the twins differs"
    assert np.array_equal(t.A.download_H(), t.B.download_H()), f"{tag}: H of the twins differs"


def still_pending(tag, t, again):
    """Behind a reader that does not rewrite H: the same bits when called again, and ``download_H`` is Hs bit for bit (the
    scale neither dropped nor applied twice)."""
    first, second = again(t.A), again(t.A)
    assert np.array_equal(first, second), f"{tag}: a second call gives other bits"
    assert np.array_equal(t.A.download_H(), t.Hs), f"{tag}: download_H behind the reader is not the materialised state"
    return first


# ------------------------------------------------------------------ readers that leave H alone: the forward evaluations


def _objective_async(e):
    e.objective_async(5)
    return e.objective_read(5, 1)[0]


@pytest.mark.parametrize("sp", grid(SOURCES), ids=sp_id)
def test_forward_readers(sp):
    """``objective``, ``objective_async`` + ``objective_read``, ``samplewise_kl``, ``reconstruct``, ``download_H``: the forward
    kernels apply the scale to the H tile they load (``fwd_params: p.hscale``), ``download_H`` flushes."""
    with twins(*sp) as t:
        tag = sp_id(sp)
        for name, fn in (("objective", lambda e: e.objective()), ("objective_async", _objective_async)):
            a, b = t.both(fn)
            check_objective(f"{tag}/{name}/A", a, t.X, t.W, t.Hs, t.wkl, t.wlh)
            assert a == b, f"{tag}/{name}: {a!r} (pending) vs {b!r} (materialised)"
            assert still_pending(f"{tag}/{name}", t, fn) == a
        assert t.A.objective() == _objective_async(t.A)  # (queued and blocking: one kernel)
        a, b = t.both(lambda e: e.samplewise_kl())
        want = orc.samplewise_kl_divergence(t.X.T, t.W.T, t.Hs.T)
        size = t.X.sum(axis=1) + (t.Hs @ t.W).sum(axis=1)
        err = np.abs(a - want)
        assert (err <= SKL_RT * np.abs(want) + SKL_ABS * size).all(), (tag, float(np.max(err / size)))
        assert np.array_equal(a, b), f"{tag}/samplewise_kl: pending and materialised differ"
        still_pending(f"{tag}/samplewise_kl", t, lambda e: e.samplewise_kl())
        a, b = t.both(lambda e: e.reconstruct())
        assert rel_l2(a, t.Hs @ t.W) < REC_L2 and np.array_equal(a, b), f"{tag}/reconstruct"
        still_pending(f"{tag}/reconstruct", t, lambda e: e.reconstruct())
        a, b = t.both(lambda e: e.download_H())
        assert np.array_equal(a, t.Hs) and np.array_equal(b, t.Hs), f"{tag}/download_H"
        assert (a >= EPS).all()
        assert np.array_equal(t.A.download_H(), t.Hs)  # flushed once, not once per download


@pytest.mark.parametrize("src", SOURCES, ids=src_id)
def test_settings_keep_the_scale_and_upload_H_drops_it(src):
    """``set_weights``, ``upload_W``, ``upload_X``, ``set_small_cohort_tiles`` and ``set_precision`` leave the scale pending;
    ``upload_H`` drops it."""
    with twins(src) as t:
        f = t.B.objective()
        wk = np.random.default_rng(3).uniform(0.5, 2.0, t.N)
        single = t.V <= 96  # (the fp32 mode refuses feature blocks)
        calls = [("set_weights", lambda e: (e.set_weights(wk, None), e.set_weights(None, None))), ("upload_W", lambda e: e.upload_W(t.W)),
                 ("upload_X", lambda e: e.upload_X(t.X)), ("set_small_cohort_tiles", lambda e: (e.set_small_cohort_tiles(64), e.set_small_cohort_tiles(0)))]
        if single:
            calls.append(("set_precision", lambda e: (e.set_precision("f32"), e.set_precision("f64"))))
        for name, call in calls:
            t.arm("A")
            call(t.A)
            assert t.A.objective() == f, f"{name}: the objective behind it is not the materialised state's"
            assert np.array_equal(t.A.download_H(), t.Hs), f"{name}: the pending scale was dropped or applied twice"
        t.arm("A")
        t.A.upload_H(t.H0)
        assert np.array_equal(t.A.download_H(), t.H0), "upload_H: the pending scale survived the upload"
        check_objective("upload_H", t.A.objective(), t.X, t.W, t.H0)


# ------------------------------------------------------------------ update_H, update_W


@pytest.mark.parametrize("sp", grid(SOURCES), ids=sp_id)
def test_update_H(sp):
    """``update_H`` applies the scale to the tile it loads, writes H in full and clears the flag."""
    with twins(*sp) as t:
        tag = sp_id(sp) + "/update_H"
        t.both(lambda e: e.update_H())
        _, Hn, _, Hp, allow = tgf.oracle_step(t.X, t.W, t.Hs, t.wkl, t.wlh, t.K)  # (H's half of the joint step is update_H)
        for e, who in ((t.A, "A"), (t.B, "B")):
            tgf.check(f"{tag}/{who}", e.download_H(), Hn, RT_STEP, pre=Hp, allowance=allow)
            assert np.array_equal(e.download_W(), t.W)
        same_state(tag, t)
        check_objective(tag, t.A.objective(), t.X, t.W, t.A.download_H(), t.wkl, t.wlh)


@pytest.mark.parametrize("clip_mode", [_lib.CLIP_NON_GIVEN, _lib.CLIP_ALL], ids=["clip_non_given", "clip_all"])
@pytest.mark.parametrize("sp", grid(SOURCES, ("fused", "wkl")), ids=sp_id)
def test_update_W(sp, clip_mode):
    """``update_W`` (the numerator pass alone applies the scale on the fly) leaves H and the pending scale alone."""
    with twins(*sp) as t:
        for g in sorted({0, min(2, t.K - 1)}):
            tag = f"{sp_id(sp)}/update_W/g{g}"
            t.both(lambda e: e.update_W(g, clip_mode))
            want = orc.update_W(t.X.T, t.W.T, t.Hs.T, t.wkl, g).T
            Wp = orc.update_WH_preclip(t.X.T, t.W.T, t.Hs.T, t.wkl, None, g)[0].T
            for e, who in ((t.A, "A"), (t.B, "B")):
                Wd = e.download_W()
                assert np.array_equal(Wd[:g], t.W[:g] if clip_mode == _lib.CLIP_NON_GIVEN else t.W[:g].clip(EPS))
                tgf.check(f"{tag}/{who}", Wd[g:], want[g:], RT_STEP, pre=Wp[g:])
            # H was not rewritten: still to be read as Hs, through the objective of the new W and through the download
            W1 = t.A.download_W()
            assert np.array_equal(W1, t.B.download_W()), tag
            check_objective(tag, t.A.objective(), t.X, W1, t.Hs, t.wkl, t.wlh)
            assert t.A.objective() == t.B.objective() and np.array_equal(t.A.download_H(), t.Hs), tag
            # and a second update from the same state gives the same bits
            t.arm("A")
            t.A.update_W(g, clip_mode)
            assert np.array_equal(t.A.download_W(), W1), f"{tag}: a second call gives other bits"


# ------------------------------------------------------------------ the joint steps


@pytest.mark.parametrize("sp", grid(SOURCES, small=True), ids=sp_id)
def test_kl_step(sp):
    """``kl_step(1)`` and ``kl_step(3)`` with 0, 2 and K given signatures: the fused joint pass flushes first (its H tiles
    travel by LDS-DMA, as they are in memory), the small-cohort kernel flushes first, the wide passes apply the scale."""
    with twins(*sp) as t:
        for n, rtol in ((1, RT_STEP), (3, RT_RUN)):
            for g in given_values(t.K):
                tag = f"{sp_id(sp)}/kl_step({n},{g})"
                t.both(lambda e: e.kl_step(n, g))
                want = oracle_steps(t, n, g)
                check_state(f"{tag}/A", t, t.A, want, rtol, g, n)
                check_state(f"{tag}/B", t, t.B, want, rtol, g, n)
                same_state(tag, t)
                check_objective(tag, t.A.objective(), t.X, t.A.download_W(), t.A.download_H(), t.wkl, t.wlh)


@pytest.mark.parametrize("src", [s for s in SOURCES if src_shape(s)[0] <= 96], ids=src_id)
def test_kl_step_f32(src):
    """The fp32 fast mode converts H as it is in memory: ``kl_steps_f32`` flushes first."""
    with twins(src, precision="f32") as t:
        tag = src_id(src) + "/f32"
        t.both(lambda e: e.kl_step(1, 0))
        want = oracle_steps(t, 1, 0)
        check_state(f"{tag}/A", t, t.A, want, RT_F32, 0)
        check_state(f"{tag}/B", t, t.B, want, RT_F32, 0)
        same_state(tag, t)


@pytest.mark.parametrize("keep", [False, True], ids=["plain", "keep"])
@pytest.mark.parametrize("sp", grid(SOURCES, small=True), ids=sp_id)
def test_kl_step_objective(sp, keep):
    """``kl_step_objective``: the objective of the state it starts from (Hs), folded into the first step's launch where the
    engine can (flushed first) and as a forward pass of its own elsewhere (scale on the fly); then the step.  ``keep``: the
    rollback returns to (W, Hs)."""
    with twins(*sp) as t:
        for g in given_values(t.K):
            tag = f"{sp_id(sp)}/kl_step_objective(g={g},keep={keep})"

            def run(e):
                e.kl_step_objective(2, 1, g, keep)
                return e.objective_read(2, 1)[0]

            a, b = t.both(run)
            check_objective(f"{tag}/A", a, t.X, t.W, t.Hs, t.wkl, t.wlh)
            assert a == b, f"{tag}: objective {a!r} (pending) vs {b!r} (materialised)"
            want = oracle_steps(t, 1, g)
            check_state(f"{tag}/A", t, t.A, want, RT_STEP, g)
            check_state(f"{tag}/B", t, t.B, want, RT_STEP, g)
            same_state(tag, t)
            if keep:
                t.A.kl_rollback(), t.B.kl_rollback()
                assert np.array_equal(t.A.download_W(), t.W) and np.array_equal(t.A.download_H(), t.Hs), f"{tag}: rollback"
                same_state(f"{tag}/rollback", t)


@pytest.mark.parametrize("sp", grid([s for s in SOURCES if src_shape(s)[0] <= 96]), ids=sp_id)
def test_kl_step_partial_and_finish(sp):
    """The split step: ``kl_step_partial`` (H and the reduced numerators, W untouched) + ``kl_step_finish``."""
    with twins(*sp) as t:
        for g in given_values(t.K):
            tag = f"{sp_id(sp)}/partial+finish(g={g})"
            t.both(lambda e: e.kl_step_partial())
            want = oracle_steps(t, 1, g)
            for e in (t.A, t.B):
                assert np.array_equal(e.download_W(), t.W), f"{tag}: the partial step changed W"
            assert np.array_equal(t.A.download_H(), t.B.download_H()), f"{tag}: H behind the partial step"
            t.A.kl_step_finish(g), t.B.kl_step_finish(g)
            check_state(f"{tag}/A", t, t.A, want, RT_STEP, g)
            check_state(f"{tag}/B", t, t.B, want, RT_STEP, g)
            same_state(tag, t)


@pytest.mark.parametrize("sp", grid(SOURCES, small=True), ids=sp_id)
def test_kl_step_keep_and_rollback(sp):
    """``kl_step_keep(2)`` + ``kl_rollback``: the kept state is the materialised one, (W, Hs) bit for bit, and a step from
    there equals the twin's."""
    with twins(*sp) as t:
        for g in given_values(t.K):
            tag = f"{sp_id(sp)}/keep(2,{g})"
            t.both(lambda e: e.kl_step_keep(2, g))
            want = oracle_steps(t, 2, g)
            check_state(f"{tag}/A", t, t.A, want, RT_RUN, g, 2)
            check_state(f"{tag}/B", t, t.B, want, RT_RUN, g, 2)
            t.arm()
            t.A.kl_step_keep(2, g), t.B.kl_step_keep(2, g)
            t.A.kl_rollback(), t.B.kl_rollback()
            assert np.array_equal(t.A.download_W(), t.W), f"{tag}: W behind the rollback"
            assert np.array_equal(t.A.download_H(), t.Hs), f"{tag}: H behind the rollback is not the materialised state"
            t.A.kl_step(1, g), t.B.kl_step(1, g)
            check_state(f"{tag}/rollback+step/A", t, t.A, oracle_steps(t, 1, g), RT_STEP, g)
            same_state(f"{tag}/rollback+step", t)


def test_cooperative_leftover_tile_with_a_scale_pending():
    """1025 tiles: a cooperative leftover tile.  ``kl_step(1)``, ``kl_step_objective`` (flushed first: the cooperative tile runs
    with and without a pending scale, the same bits) and ``update_W`` (no cooperative tile in a numerator pass alone)."""
    src = ("scale",) + S.all_cases([S.COOP_SHAPE])[0]
    with twins(src) as t:
        want = oracle_steps(t, 1, 0)
        t.both(lambda e: e.kl_step(1, 0))
        check_state("coop/kl_step/A", t, t.A, want, RT_STEP, 0)
        same_state("coop/kl_step", t)

        def run(e):
            e.kl_step_objective(1, 1, 0, False)
            return e.objective_read(1, 1)[0]

        a, b = t.both(run)
        check_objective("coop/kl_step_objective", a, t.X, t.W, t.Hs)
        assert a == b
        check_state("coop/kl_step_objective/A", t, t.A, want, RT_STEP, 0)
        same_state("coop/kl_step_objective", t)
        t.both(lambda e: e.update_W(0, _lib.CLIP_NON_GIVEN))
        Wp = orc.update_WH_preclip(t.X.T, t.W.T, t.Hs.T)[0].T
        tgf.check("coop/update_W/A", t.A.download_W(), orc.update_W(t.X.T, t.W.T, t.Hs.T).T, RT_STEP, pre=Wp)
        assert np.array_equal(t.A.download_W(), t.B.download_W()) and np.array_equal(t.A.download_H(), t.Hs)


# ------------------------------------------------------------------ MvNMF entry points, stand-alone

MV_READER_SOURCES = [("scale",) + p for p in S.all_cases([(96, 39, 7), (96, 215, 17), (96, 215, 64), (288, 215, 12)])]


MV_READER_GRID = [(s, q) for s in MV_READER_SOURCES for q in (True, False)] + [(s, s[2]) for s in MV_SOURCES]


@pytest.mark.parametrize("sq", MV_READER_GRID, ids=lambda sq: f"{src_id(sq[0])}-{'queued' if sq[1] else 'classic'}")
def test_mvnmf_readers(sq):
    """``mv_objective``, ``mv_logdet``, ``mv_update_W_unconstrained`` (H untouched), ``mv_step``, ``mv_step_objective``,
    ``mv_line_search`` (H rewritten, a new scale pending behind them), each stand-alone on a pending scale."""
    src, queued = sq
    lam, delta = 1.0, 1.0
    with twins(src, queued=queued) as t:
        tag = f"{src_id(src)}-{'queued' if queued else 'classic'}"
        Xt, Wt, Ht = t.X.T, t.W.T, t.Hs.T
        fn = lambda e: e.mv_objective(lam, delta)
        a, b = t.both(fn)
        want = orc.kl_divergence_penalized(Xt, Wt, Ht, lam, delta)
        assert np.isclose(a, want, rtol=MV_OBJ_RT, atol=0) and a == b, (tag, a, b, want)
        assert still_pending(f"{tag}/mv_objective", t, fn) == a
        fn = lambda e: e.mv_logdet(delta)
        a, b = t.both(fn)
        assert np.isclose(a, orc.volume_logdet(Wt, delta), rtol=MV_OBJ_RT, atol=0) and a == b, tag
        assert still_pending(f"{tag}/mv_logdet", t, fn) == a
        for g in sorted({0, min(2, t.K - 1)}):
            fn = lambda e: e.mv_update_W_unconstrained(g, lam, delta)
            a, b = t.both(fn)
            Wu = orc.update_W_unconstrained(Xt, Wt, Ht, lam, delta, g).T
            assert np.array_equal(a[:g], t.W[:g])
            tgf.check(f"{tag}/Wu/g{g}", a[g:], Wu[g:], RT_MV_W)
            assert np.array_equal(a, b), f"{tag}/mv_update_W_unconstrained: pending and materialised differ"
            t.arm("A")
            still_pending(f"{tag}/mv_update_W_unconstrained", t, fn)
            assert np.array_equal(t.A.download_W(), t.W)
            # mv_step and mv_step_objective
            Wn, Hn, gamma = orc.mvnmf_step(Xt, Wt, Ht, lam, delta, 1.0, g)
            a, b = t.both(lambda e: e.mv_step(1, g, lam, delta, 1.0))
            assert a == b == gamma, (tag, a, b, gamma)
            for e, who in ((t.A, "A"), (t.B, "B")):
                tgf.check(f"{tag}/mv_step/g{g}/{who}/W", e.download_W(), Wn.T, RT_MV_W)
                tgf.check(f"{tag}/mv_step/g{g}/{who}/H", e.download_H(), Hn.T, RT_MV_H)
            same_state(f"{tag}/mv_step/g{g}", t)
            a, b = t.both(lambda e: e.mv_step_objective(1, g, lam, delta, 1.0))
            assert a == b and a[0] == gamma, (tag, a, b, gamma)
            assert np.isclose(a[1], orc.kl_divergence_penalized(Xt, Wn, Hn, lam, delta), rtol=MV_STEP_OBJ_RT, atol=0), tag
            tgf.check(f"{tag}/mv_step_objective/g{g}/H", t.A.download_H(), Hn.T, RT_MV_H)
            same_state(f"{tag}/mv_step_objective/g{g}", t)
        # mv_line_search from (W, Hs) with the oracle's W_unconstrained
        Wu = orc.update_W_unconstrained(Xt, Wt, Ht, lam, delta, 0)
        Wn, Hn, gamma = orc.line_search(Xt, Wt, Ht, lam, delta, 1.0, Wu)
        a, b = t.both(lambda e: e.mv_line_search(lam, delta, 1.0, np.ascontiguousarray(Wu.T)))
        assert a == b and np.isclose(a, gamma, rtol=1e-12, atol=0), (tag, a, b, gamma)
        for e, who in ((t.A, "A"), (t.B, "B")):
            tgf.check(f"{tag}/line_search/{who}/W", e.download_W(), Wn.T, RT_MV_W)
            tgf.check(f"{tag}/line_search/{who}/H", e.download_H(), Hn.T, RT_MV_H)
        same_state(f"{tag}/line_search", t)


@pytest.mark.parametrize("name", S.MV_CHUNKED)
def test_mvnmf_step_on_signature_chunks_flushes_at_once(name):
    """K = 65 (on 96 and on 192 features): the line search of ``mv_step`` flushes at once (``if (e->NC > 1) flush_H_scale``), the
    chunked passes read H as it is.  ``objective``, ``samplewise_kl``, ``download_H`` and ``kl_step(1)`` against the twin."""
    with twins(("mv", name, True)) as t:
        a, b = t.both(lambda e: e.objective())
        check_objective(name, a, t.X, t.W, t.Hs)
        assert a == b
        a, b = t.both(lambda e: e.samplewise_kl())
        want = orc.samplewise_kl_divergence(t.X.T, t.W.T, t.Hs.T)
        size = t.X.sum(axis=1) + (t.Hs @ t.W).sum(axis=1)
        assert (np.abs(a - want) <= SKL_RT * np.abs(want) + SKL_ABS * size).all() and np.array_equal(a, b)
        a, b = t.both(lambda e: e.download_H())
        assert np.array_equal(a, t.Hs) and np.array_equal(b, t.Hs)
        t.both(lambda e: e.kl_step(1, 0))
        want = oracle_steps(t, 1, 0)
        check_state(f"{name}/kl_step/A", t, t.A, want, RT_STEP, 0)
        check_state(f"{name}/kl_step/B", t, t.B, want, RT_STEP, 0)
        same_state(f"{name}/kl_step", t)
    # and the oracle's step itself, from the uploaded state
    m = S.mv_case(name)
    assert rel_l2(t.W, m.Wn) < 1e-7 and rel_l2(t.Hs, m.Hn) < 1e-7  # (test_gpu_wide_many.py's bound for a chunked MvNMF step)


# ------------------------------------------------------------------ CorrNMF


def _corr_setup(t, dim=3):
    rng = np.random.default_rng(t.N + t.K)
    par = dict(beta=rng.normal(0.0, 0.3, t.K), alpha=np.log(t.X.sum(axis=1) / t.K) + rng.normal(0.0, 0.1, t.N),
               L=rng.normal(0.0, 0.5, (t.K, dim)), U=rng.normal(0.0, 0.5, (t.N, dim)))
    for e in (t.A, t.B):
        e.corr_configure(dim)
        for which, a in ((_lib.CORR_SIGNATURE_SCALINGS, par["beta"]), (_lib.CORR_SAMPLE_SCALINGS, par["alpha"]),
                         (_lib.CORR_SIGNATURE_EMBEDDINGS, par["L"]), (_lib.CORR_SAMPLE_EMBEDDINGS, par["U"])):
            e.corr_upload(which, a)
    return par


@pytest.mark.parametrize("src", SOURCES, ids=src_id)
def test_corrnmf_readers(src):
    """``corr_compute_aux`` (the joint fused pass with ``Hout = aux``: flushed first; on feature blocks the scale on the fly),
    ``corr_poisson_llh`` (forward kernel, scale on the fly), ``corr_update_signatures`` (the numerators of the aux pass): H
    stays; ``corr_compute_exposures`` overwrites H and discards the pending scale."""
    with twins(src) as t:
        tag = src_id(src)
        par = _corr_setup(t)
        aux_of = lambda e: (e.corr_compute_aux(), e.corr_download(_lib.CORR_AUX))[1]
        a, b = t.both(aux_of)
        assert rel_l2(a.T, co.compute_aux(t.X, t.W, t.Hs)) < CORR_BOUND and np.array_equal(a, b), f"{tag}/aux"
        assert np.array_equal(still_pending(f"{tag}/aux", t, aux_of), a)
        a, b = t.both(lambda e: e.corr_poisson_llh())
        want = co.poisson_llh(t.X.T, t.W.T, t.Hs.T)
        assert abs(a - want) <= CORR_BOUND * abs(want) and a == b, (tag, a, b, want)
        assert still_pending(f"{tag}/llh", t, lambda e: e.corr_poisson_llh()) == a
        g = min(2, t.K - 1)

        def update_signatures(e):
            e.corr_compute_aux(), e.corr_update_signatures(g)
            return e.download_W()

        a, b = t.both(update_signatures)
        assert rel_l2(a, orc.update_W(t.X.T, t.W.T, t.Hs.T, n_given_signatures=g).T) < CORR_BOUND and np.array_equal(a, b), f"{tag}/signatures"
        assert np.array_equal(a[:g], t.W[:g])
        assert np.array_equal(t.A.download_H(), t.Hs), f"{tag}/signatures: H behind the update"
        t.arm("A")
        assert np.array_equal(update_signatures(t.A), a), f"{tag}/signatures: a second run gives other bits"
        # compute_exposures: H overwritten in full, the scale is gone
        a, b = t.both(lambda e: (e.corr_compute_exposures(), e.download_H())[1])
        assert rel_l2(a, co.compute_exposures(par["beta"], par["alpha"], par["L"], par["U"])) < CORR_BOUND and np.array_equal(a, b), f"{tag}/exposures"
        assert t.A.objective() == t.B.objective()


# ------------------------------------------------------------------ composition


@pytest.mark.parametrize("src", SOURCES, ids=src_id)
def test_a_second_scale_on_top_of_a_pending_one(src):
    """``set_H_scale`` on a pending scale (of ``set_H_scale``, of an MvNMF step) materialises the earlier one first: H reads
    as ``clip(clip(H0 s1) s2)``, bit for bit."""
    with twins(src) as t:
        s2 = S.case(*src[1:]).scale2 if src[0] == "scale" else S.make_scale(t.K, 7 + t.K)
        H2 = S.compose(t.Hs, s2)
        tag = src_id(src) + "/composition"

        def arm2():
            t.arm("A")
            t.A.set_H_scale(s2)
            t.B.upload_W(t.W), t.B.upload_H(H2)

        arm2()
        assert np.array_equal(t.A.download_H(), H2), f"{tag}: download_H is not clip(clip(H0 s1) s2)"
        arm2()
        a, b = t.A.objective(), t.B.objective()
        check_objective(tag, a, t.X, t.W, H2)
        assert a == b
        t.A.kl_step(1, 0), t.B.kl_step(1, 0)
        want = oracle_steps(t, 1, 0, H=H2)
        check_state(f"{tag}/kl_step/A", t, t.A, want, RT_STEP, 0)
        same_state(f"{tag}/kl_step", t)
