"""Case tables and oracle side of ``tests/test_gpu_engine_rotation.py`` (checked on the host by ``test_rotation_ref_host.py``).

Since the paired leftover round (``salnmf_fused_kernel.h``: the pairing rule) a joint step of a *pairing* shape --
``tiles = 4 grid + L`` with ``0 < 2 L <= grid`` -- writes the new H to a third buffer and the buffers change roles
(``salnmf.hip: kl_step_once``).  ``e->H`` may then name any of three allocations, with the kept state of
``kl_step_keep``, MvNMF's speculation, a pending scale and a half step held across a call on top.

**The invariant.**  The observable state of an engine is X, W and H as the downloads return them, the weights and the
mode switches.  Engine A reaches a state by a *prefix* that rotated buffers, engine B is fresh with A's downloaded W and
H uploaded; both get the same *probe*.  A and B return the same bits and hold the same bits afterwards, and the result
meets the probe's oracle reference at the tolerance of the file that owns the entry point.

A prefix and a probe are lists of *ops*, ``(method name, arguments...)``: the device test calls them on an ``Engine``,
:func:`oracle_run` follows them with ``oracle.klnmf_oracle`` on a host state.  ``mark`` / ``back_to_mark`` are not calls: they
hold the exact return of a rollback (the device test downloads and compares bits, the oracle ignores them).
"""

from __future__ import annotations

import functools
from dataclasses import dataclass, field, replace

import numpy as np

import _corr_ref as R
import _f32_ref as fr
import _scale_ref as S
from oracle import corrnmf_oracle as co
from oracle import klnmf_oracle as orc

# ------------------------------------------------------------------ tolerances: none is new, each belongs to another file
TOL = 1e-10            # test_gpu_parity.py: TOL; per entry as in test_gpu_coop_roles.py (np.allclose(rtol=TOL, atol=0))
OBJ_RTOL = 1e-12       # test_gpu_parity.py: test_objective_folded_into_the_following_step, test_shapes_one_and_five_steps
SKL_RTOL = 1e-10       # test_gpu_parity.py: test_shapes_one_and_five_steps (samplewise_kl)
REC_RTOL = 1e-13       # test_gpu_parity.py: test_shapes_one_and_five_steps (reconstruct)
MV_L2 = 1e-7           # test_gpu_parity.py: test_every_signature_count (rel-L2 of W and H behind an MvNMF step)
MV_GAMMA_RTOL = 1e-12  # test_gpu_parity.py: test_golden_mvnmf (gammas)
MV_OBJ_RTOL = 1e-11    # test_gpu_parity.py: test_golden_mvnmf (mv_objective), test_mvnmf_function_level_api
MV_STEP_OBJ_RTOL = 1e-9  # test_gpu_parity.py: test_mv_step_returns_the_objective_of_the_state_it_leaves
MV_LOGDET_RTOL = 1e-11  # test_gpu_wide.py: test_wide_mvnmf_steps_and_function_level_api_match_the_oracle (mv_logdet)
CORR_RTOL = 1e-12      # test_gpu_corrnmf.py: RTOL (aux by rel-L2, the likelihood relative)
# fp32: _f32_ref.bound_H / bound_W through _f32_ref.check (test_gpu_fast_entrywise.py)
# exposures of CorrNMF: _corr_ref.C["H"] units of _corr_ref.compute_exposures (test_gpu_corr_entrywise.py)

LAM, DELTA, GAMMA0 = 1.0, 1.0, 1.0  # the MvNMF ops
CORR_DIM = 3
RAGGED = 5

# ------------------------------------------------------------------ shapes


def leftover(which, g):
    return {"one": 1, "half": g // 2, "half+1": g // 2 + 1}[which]


def form(L, g):
    """As ``test_gpu_coop_roles.form``."""
    return "paired" if 2 * L <= g else ("single" if L <= g else "plain")


def samples(which, g):
    return 16 * (4 * g + leftover(which, g)) - RAGGED


@dataclass(frozen=True)
class Shape:
    V: int
    K: int
    which: str
    form: str
    note: str

    @property
    def id(self):
        return f"V{self.V}-K{self.K}-L{self.which}"


PRIMARY = Shape(96, 50, "half", "paired", "takes the full prefix x probe cross")
PAIRING = [
    PRIMARY,
    Shape(96, 50, "one", "paired", "one pair"),
    Shape(96, 20, "half", "paired", "geometry (8, 1, 4)"),
    Shape(96, 5, "half", "paired", "geometry (2, 1, 0)"),
    Shape(83, 30, "half", "paired", "masked feature columns"),
]
CONTROL = Shape(96, 50, "half+1", "single", "the one-workgroup form, in place")
SHAPES = PAIRING + [CONTROL]

# ------------------------------------------------------------------ the tables

PREFIXES = {
    "P0": [],
    "P1": [("kl_step", 1)],
    "P2": [("kl_step", 2)],
    "P3": [("kl_step", 1), ("kl_step_keep", 2)],
    "P4": [("kl_step", 1), ("mark",), ("kl_step_keep", 1), ("kl_rollback",), ("back_to_mark",)],
    "P5": [("kl_step", 1), ("mark",), ("kl_step_objective", 0, 2, 0, True), ("kl_rollback",), ("back_to_mark",)],
    "P6q": [("set_mv_queued", True), ("kl_step", 1), ("mv_step", 2), ("kl_step", 1)],
    "P6c": [("set_mv_queued", False), ("kl_step", 1), ("mv_step", 2), ("kl_step", 1)],
    "P7": [("kl_step", 1), ("mv_step_objective", 1, True)],
    "P8": [("kl_step", 1), ("set_H_scale",)],
    "P9": [("kl_step", 1), ("kl_step", 1, "K"), ("kl_step", 1)],
    "P10": [("kl_step", 1), ("set_weights", True), ("kl_step", 1), ("set_weights", False)],
    "P11": [("kl_step", 1), ("set_precision", "f32"), ("kl_step", 1), ("set_precision", "f64")],
    "P12": [("kl_step", 1), ("upload_H",)],
    "P13": [("kl_step", 1), ("set_persistent", True), ("kl_step_keep", 2), ("set_persistent", False)],
}
NEEDS_PERSISTENT = {"P13"}  # skipped, with that reason, where the build carries no persistent kernel

PROBES = {
    "kl_step1": [("kl_step", 1)],
    "kl_step2": [("kl_step", 2)],
    "keep_rollback": [("mark",), ("kl_step_keep", 1), ("kl_rollback",), ("back_to_mark",), ("kl_step", 1)],
    "step_objective": [("kl_step_objective", 3, 2, 0, False), ("objective_read", 3)],
    "update_H": [("update_H",)],
    "update_W": [("update_W", 2)],
    "objective": [("objective",)],
    "samplewise_kl": [("samplewise_kl",)],
    "reconstruct": [("reconstruct",)],
    "mv_step": [("mv_step", 1)],
    "mv_ahead_then_kl": [("mv_step_objective", 1, True), ("kl_step", 1)],
    "mv_objective": [("mv_objective",)],
    "mv_logdet": [("mv_logdet",)],
    "partial_finish": [("kl_step_partial",), ("w_unchanged",), ("kl_step_finish",)],
    "f32_step": [("set_precision", "f32"), ("kl_step", 1)],
    "weights_step": [("set_weights", True), ("kl_step", 1)],
    "corr": [("corr_configure",), ("corr_upload",), ("corr_compute_exposures",), ("download_H",), ("corr_compute_aux",), ("corr_download",),
             ("corr_poisson_llh",), ("kl_step", 1)],
}
# ops of the harness itself that are no Engine methods
PSEUDO = {"mark", "back_to_mark", "w_unchanged"}
# Engine methods the harness calls around every case
HARNESS = {
    "upload_X": "every engine of a case",
    "upload_W": "every engine of a case; B takes A's downloaded W",
    "download_W": "the observable state",
    "fused_grid": "the shapes are computed from it",
    "device_ptr": "test_the_step_moves_H_on_a_pairing_shape_only",
}
# ... and the ones these tables leave to other files
EXEMPT = {
    "close": "lifetime",
    "sync": "a stream synchronisation, touches no buffer",
    "profile_kl_steps": "measurement aid (runs kl_step_once, which the kl_step ops cover)",
    "profile_sharded_steps": "measurement aid of sharded engines",
    "profile_objective": "measurement aid",
    "profile_reconstruct": "measurement aid",
    "comm_unique_id": "multi-process engines are out of scope",
    "comm_init": "multi-process engines are out of scope",
    "comm_info": "multi-process engines are out of scope",
    "comm_observed": "multi-process engines are out of scope",
    "p2p_export": "needs peers",
    "p2p_connect": "needs peers",
    "set_p2p_timeout": "needs peers",
    "set_p2p": "needs peers",
    "init_gram": "pinned by test_gpu_init_entrywise.py",
    "init_project": "pinned by test_gpu_init_entrywise.py",
    "init_finish": "pinned by test_gpu_init_entrywise.py",
    "init_separable": "pinned by test_gpu_init_entrywise.py",
    "init_flat": "pinned by test_gpu_init_entrywise.py",
    "objective_async": "the launch of objective with another destination (test_gpu_pending_scale.py holds the two to one value)",
    "mv_update_W_unconstrained": "the first half of mv_step, which is a probe",
    "mv_line_search": "the second half of mv_step, which is a probe",
    "mv_update_W": "the W half of mv_step, which is a probe",
    "set_lockstep": "chooses a CorrNMF embedding solver, no reader of H",
    "set_batched_sample_solves": "chooses a CorrNMF embedding solver, no reader of H",
    "set_w_dma": "how W reaches LDS, not where H lives",
    "set_small_cohort_tiles": "no shape that pairs has few enough tiles for the one-workgroup kernel",
    "corr_update_sample_scalings": "reads X and the embeddings, not H",
    "corr_update_signature_scalings": "reads aux, not H",
    "corr_update_signatures": "reads the numerators corr_compute_aux left, not H",
    "corr_update_sample_embeddings": "reads aux, not H",
    "corr_update_sample_embeddings_multi": "reads aux, not H",
    "corr_update_signature_embeddings": "reads aux, not H",
    "corr_update_signature_embeddings_from": "reads caller-gathered inputs",
    "corr_embedding_sumsq": "reads the embeddings",
}


def table_methods():
    """Every Engine method an op of the tables names."""
    return {op[0] for ops in list(PREFIXES.values()) + list(PROBES.values()) for op in ops} - PSEUDO


def cases():
    """``(shape, prefix id, probe id)``: the full cross on the primary shape; on the other shapes every prefix once (with
    ``kl_step2``) and every probe once (behind P1)."""
    out = [(PRIMARY, p, q) for p in PREFIXES for q in PROBES]
    for s in SHAPES:
        if s is PRIMARY:
            continue
        out += [(s, p, "kl_step2") for p in PREFIXES]
        out += [(s, "P1", q) for q in PROBES if q != "kl_step2"]
    return out


def case_id(c):
    return f"{c[0].id}-{c[1]}-{c[2]}"


# ------------------------------------------------------------------ a shape's inputs


@dataclass(frozen=True)
class Inputs:
    shape: Shape
    g: int
    N: int
    X: np.ndarray       # (N, V)
    W0: np.ndarray      # (K, V)
    H0: np.ndarray      # (N, K)
    scale: np.ndarray   # (K,) set_H_scale: _scale_ref.make_scale
    wkl: np.ndarray
    wlh: np.ndarray
    Hup: np.ndarray     # upload_H of P12
    corr: dict          # beta, alpha, L, U


@functools.lru_cache(maxsize=8)
def inputs(shape: Shape, g: int) -> Inputs:
    V, K = shape.V, shape.K
    L = leftover(shape.which, g)
    N = samples(shape.which, g)
    X, W0, H0 = orc.synthetic_problem(V, N, K, seed=V + K + L)
    rng = np.random.default_rng(7 + V + K)
    wkl, wlh = rng.uniform(0.5, 2.0, N), rng.uniform(0.0, 0.3, N)  # (test_gpu_coop_roles.run_case)
    Hup = np.ascontiguousarray(H0[::-1] * rng.uniform(0.5, 1.5, (N, K)))
    corr = dict(beta=rng.normal(0.0, 0.3, K), alpha=np.log(X.sum(axis=1) / K) + rng.normal(0.0, 0.1, N),
                L=rng.normal(0.0, 0.5, (K, CORR_DIM)), U=rng.normal(0.0, 0.5, (N, CORR_DIM)))  # (test_gpu_corrnmf.synthetic)
    scale = S.make_scale(K, 1000 + V + N + K)
    for a in (X, W0, H0, scale, wkl, wlh, Hup, *corr.values()):
        a.setflags(write=False)
    return Inputs(shape, g, N, X, W0, H0, scale, wkl, wlh, Hup, corr)


# ------------------------------------------------------------------ the oracle's state and its ops


@dataclass(frozen=True)
class State:
    W: np.ndarray  # (K, V)
    H: np.ndarray  # (N, K)
    weights: bool = False
    fast: bool = False
    kept: tuple | None = None
    mark: tuple | None = None
    gamma: float = GAMMA0
    slots: dict = field(default_factory=dict)
    # what the last writer of (W, H) was held to: "f64" (TOL per entry), "mv" (MV_L2), "f32" (_f32_ref.check with ``pre``)
    kind: str = "f64"
    pre: tuple | None = None  # (H_pre, W_pre, T_w) of an fp32 step


@dataclass(frozen=True)
class Returned:
    op: str
    value: object
    check: str  # "objective", "skl", "reconstruct", "gamma", "mv_step_objective", "mv_objective", "mv_logdet", "corr_H", "aux", "llh"
    unit: object = None


def _weights(inp, st):
    return (inp.wkl, inp.wlh) if st.weights else (None, None)


def _worse(a, b):
    order = ("f64", "mv", "f32")
    return order[max(order.index(a), order.index(b))]


def _steps(inp, st, n, g):
    wk, wl = _weights(inp, st)
    if st.fast:
        assert n == 1 and not st.weights
        Hn, Wn, Hp, Wp = fr.exact_step(inp.X, st.W, st.H, g)
        return replace(st, W=Wn, H=Hn, kind="f32", pre=(Hp, Wp, fr.tiles_per_wave(inp.N, inp.g)))
    W, H = st.W.T, st.H.T
    for _ in range(n):
        W, H = orc.update_WH(inp.X.T, W, H, wk, wl, g)
    return replace(st, W=np.ascontiguousarray(W.T), H=np.ascontiguousarray(H.T), pre=None)


def _mv(inp, st, n):
    W, H, gamma = st.W.T, st.H.T, GAMMA0  # (every call starts its line search from GAMMA0, on the device too)
    for _ in range(n):
        W, H, gamma = orc.mvnmf_step(inp.X.T, W, H, LAM, DELTA, gamma, 0)
    return replace(st, W=np.ascontiguousarray(W.T), H=np.ascontiguousarray(H.T), gamma=float(gamma), kept=None, kind=_worse(st.kind, "mv"), pre=None)


def oracle_op(inp: Inputs, st: State, op):
    """``(state behind the op, [Returned ...])``."""
    name, args = op[0], op[1:]
    K = inp.shape.K
    Xt = inp.X.T
    wk, wl = _weights(inp, st)
    if name in ("mark", "back_to_mark", "w_unchanged", "set_mv_queued", "set_persistent", "corr_configure", "corr_upload", "corr_compute_aux",
                "kl_step_partial"):
        if name == "mark":
            return replace(st, mark=(st.W, st.H)), []
        if name == "back_to_mark":
            assert st.W is st.mark[0] and st.H is st.mark[1]
        return st, []
    if name == "kl_step":
        g = K if len(args) > 1 and args[1] == "K" else (args[1] if len(args) > 1 else 0)
        return _steps(inp, st, args[0], g), []
    if name == "kl_step_finish":  # (behind kl_step_partial: the two are one joint step)
        return _steps(inp, st, 1, 0), []
    if name == "kl_step_keep":
        return replace(_steps(inp, st, args[0], 0), kept=(st.W, st.H, st.kind, st.pre)), []
    if name == "kl_rollback":
        if st.kept is None:
            raise RuntimeError("no kept state")
        return replace(st, W=st.kept[0], H=st.kept[1], kind=st.kept[2], pre=st.kept[3], kept=None), []
    if name == "kl_step_objective":
        slot, n, g, keep = args
        f = orc.klnmf_objective(Xt, st.W.T, st.H.T, wk, wl)
        new = _steps(inp, st, n, g)
        new = replace(new, slots={**st.slots, slot: f}, kept=(st.W, st.H, st.kind, st.pre) if keep else st.kept)
        return new, []
    if name == "objective_read":
        return st, [Returned(name, st.slots[args[0]], "objective")]
    if name == "mv_step":
        new = _mv(inp, st, args[0])
        return new, [Returned(name, new.gamma, "gamma")]
    if name == "mv_step_objective":
        new = _mv(inp, st, args[0])
        f = orc.kl_divergence_penalized(Xt, new.W.T, new.H.T, LAM, DELTA)
        return new, [Returned(name, (new.gamma, f), "mv_step_objective")]
    if name == "set_H_scale":
        return replace(st, H=S.materialise(st.H, inp.scale)), []
    if name == "set_weights":
        return replace(st, weights=bool(args[0])), []
    if name == "set_precision":
        return replace(st, fast=args[0] == "f32"), []
    if name == "upload_H":
        return replace(st, H=inp.Hup, kept=None, kind="f64" if st.kind != "mv" else "mv", pre=None), []
    if name == "update_H":
        return replace(st, H=np.ascontiguousarray(orc.update_H(Xt, st.W.T, st.H.T, wk, wl).T), pre=None), []
    if name == "update_W":
        return replace(st, W=np.ascontiguousarray(orc.update_W(Xt, st.W.T, st.H.T, wk, args[0]).T), pre=None), []
    if name == "objective":
        return st, [Returned(name, orc.klnmf_objective(Xt, st.W.T, st.H.T, wk, wl), "objective")]
    if name == "samplewise_kl":
        return st, [Returned(name, orc.samplewise_kl_divergence(Xt, st.W.T, st.H.T), "skl")]
    if name == "reconstruct":
        return st, [Returned(name, st.H @ st.W, "reconstruct")]
    if name == "mv_objective":
        return st, [Returned(name, orc.kl_divergence_penalized(Xt, st.W.T, st.H.T, LAM, DELTA), "mv_objective")]
    if name == "mv_logdet":
        return st, [Returned(name, orc.volume_logdet(st.W.T, DELTA), "mv_logdet")]
    if name == "corr_compute_exposures":
        return st, []  # (the value arrives with download_H: the probe's next op)
    if name == "download_H":  # behind corr_compute_exposures only
        c = inp.corr
        return st, [Returned(name, co.compute_exposures(c["beta"], c["alpha"], c["L"], c["U"]), "corr_H")]
    if name == "corr_download":  # aux of the exposures the device itself computed: the reference is formed by the device test
        return st, [Returned(name, None, "aux")]
    if name == "corr_poisson_llh":
        return st, [Returned(name, None, "llh")]
    raise KeyError(name)


def oracle_run(inp: Inputs, st: State, ops):
    out = []
    for op in ops:
        st, r = oracle_op(inp, st, op)
        out += r
    return st, out


def start_state(inp: Inputs) -> State:
    return State(inp.W0, inp.H0)


@functools.lru_cache(maxsize=128)
def prefix_state(shape: Shape, g: int, prefix: str) -> State:
    """The oracle's state behind a prefix, from the shape's seeded start."""
    inp = inputs(shape, g)
    return oracle_run(inp, start_state(inp), PREFIXES[prefix])[0]


@functools.lru_cache(maxsize=8)
def corr_exposures_ld(shape: Shape, g: int):
    """``(H, unit)`` in extended precision (``_corr_ref.compute_exposures``): what ``test_gpu_corr_entrywise.py`` holds H to."""
    c = inputs(shape, g).corr
    return R.compute_exposures(c["beta"], c["alpha"], c["L"], c["U"])


# ------------------------------------------------------------------ comparisons (host arrays only: shared by both tests)


def entry_error(got, want):
    """Largest ``|got - want| / |want|``."""
    got, want = np.asarray(got, dtype=np.float64), np.asarray(want, dtype=np.float64)
    with np.errstate(divide="ignore", invalid="ignore"):
        r = np.abs(got - want) / np.abs(want)
    return float(np.nanmax(np.where(got == want, 0.0, r))) if r.size else 0.0


def check_state(tag, W, H, st: State, start=None):
    """The device's (W, H) against the oracle's state ``st`` at the tolerance of its last writer; returns the largest error in
    units of that tolerance's own measure (entry error for f64, rel-L2 for mv, share of the bound for f32)."""
    if st.kind == "f64":
        eW, eH = entry_error(W, st.W), entry_error(H, st.H)
        assert np.allclose(W, st.W, rtol=TOL, atol=0), f"{tag}: W is {eW:.2e} off in an entry (TOL {TOL})"
        assert np.allclose(H, st.H, rtol=TOL, atol=0), f"{tag}: H is {eH:.2e} off in an entry (TOL {TOL})"
        return max(eW, eH)
    if st.kind == "mv":
        eW = float(np.linalg.norm(W - st.W) / np.linalg.norm(st.W))
        eH = float(np.linalg.norm(H - st.H) / np.linalg.norm(st.H))
        assert eW < MV_L2 and eH < MV_L2, f"{tag}: rel-L2 W {eW:.2e} H {eH:.2e} behind an MvNMF step (bound {MV_L2})"
        return max(eW, eH)
    K, V = st.W.shape
    Hp, Wp, T_w = st.pre
    rh = fr.check(H, st.H, Hp, fr.bound_H(K, V), f"{tag}/H")
    rw = fr.check(W, st.W, Wp, fr.bound_W(K, T_w), f"{tag}/W")
    return max(rh, rw)


def check_returned(tag, got, ref: Returned):
    """One returned value against its reference; returns the relative error."""
    c, want = ref.check, ref.value
    if c in ("objective", "mv_objective", "mv_logdet"):
        rtol = {"objective": OBJ_RTOL, "mv_objective": MV_OBJ_RTOL, "mv_logdet": MV_LOGDET_RTOL}[c]
        assert np.isclose(got, want, rtol=rtol, atol=0), f"{tag}/{ref.op}: {got!r} vs {want!r}"
        return abs(got - want) / abs(want)
    if c == "gamma":
        assert np.isclose(got, want, rtol=MV_GAMMA_RTOL, atol=0), f"{tag}/{ref.op}: gamma {got!r} vs {want!r}"
        return abs(got - want) / abs(want)
    if c == "mv_step_objective":
        assert np.isclose(got[0], want[0], rtol=MV_GAMMA_RTOL, atol=0), f"{tag}/{ref.op}: gamma {got[0]!r} vs {want[0]!r}"
        assert np.isclose(got[1], want[1], rtol=MV_STEP_OBJ_RTOL, atol=0), f"{tag}/{ref.op}: objective {got[1]!r} vs {want[1]!r}"
        return abs(got[1] - want[1]) / abs(want[1])
    if c == "skl":
        assert np.allclose(got, want, rtol=SKL_RTOL, atol=0), f"{tag}/{ref.op}: {entry_error(got, want):.2e}"
        return entry_error(got, want)
    if c == "reconstruct":
        assert np.allclose(got, want, rtol=REC_RTOL, atol=0), f"{tag}/{ref.op}: {entry_error(got, want):.2e}"
        return entry_error(got, want)
    raise KeyError(c)
