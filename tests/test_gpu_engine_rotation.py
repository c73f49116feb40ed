"""Every engine entry point behind a rotation of H's buffers, against a fresh engine (DESIGN.md section 4.8 is the table this
file enforces; ``tests/_rotation_ref.py`` holds the cases, the oracle side and the tolerances, none of which is new).

A joint step of a pairing shape (``tiles = 4 grid + L``, ``0 < 2 L <= grid``) writes the new H to a third buffer and swaps.
The kernel's freedom from races rests on that host rule, and the rest of the host has to cope with ``e->H`` naming any of
three allocations.  Per case ``(shape, prefix, probe)``, with twin engines:

* A2 runs the prefix and is downloaded: its (W, H) meet the oracle's state behind the same calls, and P4 / P5 return the bits
  they kept.  (A itself is not downloaded: a download materialises a pending scale and settles a half step held across a
  call, which are arrangements the probe is to meet.)
* A runs the prefix; B is fresh, with A2's downloaded W and H uploaded and the modes the prefix leaves.
* Both get the probe.  What they return and what they hold afterwards is equal bit for bit -- both run the same kernel form
  on the same shape from the same observable state -- and meets the oracle's result from that state.

Run with ``-s``: each case prints ``ROTMAX tag value``, its largest error against the oracle in the unit of its tolerance.
"""

import functools

import numpy as np
import pytest

import _rotation_ref as RR
from oracle import corrnmf_oracle as co
from salamander_amd import Engine, _lib

pytestmark = pytest.mark.gpu

NO_KEPT_STATE = "no kept state"  # salnmf.hip: salnmf_kl_rollback


@functools.lru_cache(maxsize=None)
def grid():
    """The workgroups of the update passes on this device, as an engine with more than four tiles per workgroup reports them."""
    e = Engine(16 * 4 * 512, 96, 1)
    g = e.fused_grid()
    e.close()
    assert g < 512
    return g


@functools.lru_cache(maxsize=None)
def persistent_built():
    return bool(_lib.load().salnmf_build_flags() & _lib.BUILD_PERSISTENT)


def new_engine(inp, W=None, H=None):
    s = inp.shape
    e = Engine(inp.N, s.V, s.K)
    assert e.fused_grid() == inp.g
    e.upload_X(inp.X), e.upload_W(inp.W0 if W is None else W), e.upload_H(inp.H0 if H is None else H)
    return e


def call(e, op, inp, env, checks):
    """One op on an engine; ``(returned?, value)``."""
    name, args = op[0], op[1:]
    K = inp.shape.K
    if name in RR.PSEUDO:
        if not checks:
            return False, None
        W, H = e.download_W(), e.download_H()
        if name == "mark":
            env["mark"] = (W, H)
        elif name == "back_to_mark":
            assert np.array_equal(W, env["mark"][0]) and np.array_equal(H, env["mark"][1]), "the rollback did not restore the kept bits"
        else:
            assert np.array_equal(W, env["start"][0]), "kl_step_partial changed W"
        return False, None
    if name == "kl_step":
        e.kl_step(args[0], K if len(args) > 1 and args[1] == "K" else (args[1] if len(args) > 1 else 0))
    elif name == "kl_step_keep":
        e.kl_step_keep(args[0])
    elif name == "kl_step_objective":
        e.kl_step_objective(*args)
    elif name == "objective_read":
        return True, float(e.objective_read(args[0], 1)[0])
    elif name == "mv_step":
        return True, e.mv_step(args[0], 0, RR.LAM, RR.DELTA, RR.GAMMA0)
    elif name == "mv_step_objective":
        return True, e.mv_step_objective(args[0], 0, RR.LAM, RR.DELTA, RR.GAMMA0, args[1])
    elif name == "set_H_scale":
        e.set_H_scale(inp.scale)
    elif name == "set_weights":
        e.set_weights(*((inp.wkl, inp.wlh) if args[0] else (None, None)))
    elif name == "upload_H":
        e.upload_H(inp.Hup)
    elif name == "update_W":
        e.update_W(args[0], _lib.CLIP_NON_GIVEN)
    elif name in ("mv_objective",):
        return True, e.mv_objective(RR.LAM, RR.DELTA)
    elif name == "mv_logdet":
        return True, e.mv_logdet(RR.DELTA)
    elif name == "corr_configure":
        e.corr_configure(RR.CORR_DIM)
    elif name == "corr_upload":
        c = inp.corr
        for which, a in ((_lib.CORR_SIGNATURE_SCALINGS, c["beta"]), (_lib.CORR_SAMPLE_SCALINGS, c["alpha"]), (_lib.CORR_SIGNATURE_EMBEDDINGS, c["L"]),
                         (_lib.CORR_SAMPLE_EMBEDDINGS, c["U"])):  # (test_gpu_corrnmf.engine_from)
            e.corr_upload(which, a)
    elif name == "corr_download":
        return True, e.corr_download(_lib.CORR_AUX)
    elif name in ("objective", "samplewise_kl", "reconstruct", "download_H", "corr_poisson_llh"):
        return True, getattr(e, name)()
    else:  # no arguments beyond the table's, nothing returned
        getattr(e, name)(*args)
    return False, None


def run(e, ops, inp, start=None, checks=True):
    env, out = {"start": start}, []
    for op in ops:
        returned, value = call(e, op, inp, env, checks)
        if returned:
            out.append(value)
    return out


def modes_left(ops):
    """The mode switches a prefix leaves behind, as ops for the fresh engine (every prefix puts weights, precision and the
    persistent launch back; P6c leaves the classic MvNMF form on)."""
    last = {}
    for op in ops:
        if op[0] in ("set_mv_queued", "set_weights", "set_precision", "set_persistent"):
            last[op[0]] = op
    assert all(op in (("set_weights", False), ("set_precision", "f64"), ("set_persistent", False)) or op[0] == "set_mv_queued" for op in last.values())
    return [op for op in last.values() if op[0] == "set_mv_queued"]


def same_bits(a, b):
    if isinstance(a, tuple):
        return len(a) == len(b) and all(same_bits(x, y) for x, y in zip(a, b))
    return np.array_equal(np.asarray(a), np.asarray(b))


def skip_unless_built(prefix):
    if prefix in RR.NEEDS_PERSISTENT and not persistent_built():
        pytest.skip("this build carries no persistent kernel (SALNMF_WITH_PERSISTENT=1 adds it)")


def after_prefix(inp, prefix, tag):
    """A2: the prefix with its checks, downloaded and held to the oracle; returns (W, H) and the error."""
    a2 = new_engine(inp)
    try:
        run(a2, RR.PREFIXES[prefix], inp)
        Ws, Hs = a2.download_W(), a2.download_H()
    finally:
        a2.close()
    err = RR.check_state(f"{tag}/prefix", Ws, Hs, RR.prefix_state(inp.shape, inp.g, prefix))
    return Ws, Hs, err


def check_probe(tag, inp, probe, start, got, WA, HA):
    """What A returned and holds against the oracle's probe from the state A2 downloaded; the largest error."""
    Ws, Hs = start
    st0 = RR.State(Ws, Hs)
    ops = RR.PROBES[probe]
    worst = 0.0
    if probe == "corr":
        Hdev, aux, llh = got
        Hld, unit = RR.corr_exposures_ld(inp.shape, inp.g)
        ratio, where = RR.R.rel_ratio(Hdev, Hld, unit)
        assert ratio <= RR.R.C["H"], f"{tag}: exposures at {where} are {ratio:.2f} units off, allowed {RR.R.C['H']:.2f}"  # test_gpu_corr_entrywise.py
        want = co.compute_aux(inp.X, Ws, Hdev)  # (K, N), from the exposures the device itself holds
        e_aux = float(np.linalg.norm(aux.T - want) / np.linalg.norm(want))
        want = co.poisson_llh(inp.X.T, Ws.T, Hdev.T)
        e_llh = abs(llh - want) / abs(want)
        assert e_aux < RR.CORR_RTOL and e_llh <= RR.CORR_RTOL, f"{tag}: aux {e_aux:.2e} llh {e_llh:.2e}"  # test_gpu_corrnmf.py: RTOL
        st0, ops = RR.State(Ws, Hdev), [("kl_step", 1)]
        got = []
        worst = max(e_aux, e_llh)
    st, refs = RR.oracle_run(inp, st0, ops)
    assert len(refs) == len(got), (tag, len(refs), len(got))
    for value, ref in zip(got, refs):
        worst = max(worst, RR.check_returned(tag, value, ref))
    if probe == "update_W":
        assert np.array_equal(WA[:2], Ws[:2]), f"{tag}: the given signatures moved"
    return max(worst, RR.check_state(f"{tag}/probe", WA, HA, st))


@pytest.mark.parametrize("case", RR.cases(), ids=RR.case_id)
def test_probe_behind_a_prefix_equals_the_probe_on_a_fresh_engine(case):
    shape, prefix, probe = case
    skip_unless_built(prefix)
    tag = RR.case_id(case)
    g = grid()
    assert RR.form(RR.leftover(shape.which, g), g) == shape.form
    inp = RR.inputs(shape, g)
    Ws, Hs, err_prefix = after_prefix(inp, prefix, tag)
    a = b = None
    try:
        a = new_engine(inp)
        run(a, RR.PREFIXES[prefix], inp, checks=False)
        b = new_engine(inp, Ws, Hs)
        run(b, modes_left(RR.PREFIXES[prefix]), inp)
        ra = run(a, RR.PROBES[probe], inp, start=(Ws, Hs))
        rb = run(b, RR.PROBES[probe], inp, start=(Ws, Hs))
        WA, HA, WB, HB = a.download_W(), a.download_H(), b.download_W(), b.download_H()
    finally:
        for e in (a, b):
            if e is not None:
                e.close()
    assert len(ra) == len(rb)
    for i, (x, y) in enumerate(zip(ra, rb)):
        assert same_bits(x, y), f"{tag}: returned value {i} differs between the twins: {x!r} vs {y!r}"
    assert np.array_equal(WA, WB), f"{tag}: W of the twins differs in {int((WA != WB).sum())} entries"
    assert np.array_equal(HA, HB), f"{tag}: H of the twins differs in {int((HA != HB).sum())} entries"
    err_probe = check_probe(tag, inp, probe, (Ws, Hs), ra, WA, HA)
    print(f"ROTMAX {tag} prefix {err_prefix:.3e} probe {err_probe:.3e}")


@pytest.mark.parametrize("shape", RR.SHAPES, ids=lambda s: s.id)
def test_the_step_moves_H_on_a_pairing_shape_only(shape):
    """Non-vacuity on the device: behind ``kl_step(1)`` ``device_ptr(BUF_H)`` names another allocation on a pairing shape and
    the same one on the control shape; a second step returns to the first buffer, an all-given step stays where it is."""
    g = grid()
    inp = RR.inputs(shape, g)
    e = new_engine(inp)
    try:
        p0 = e.device_ptr(_lib.BUF_H)
        e.kl_step(1)
        p1 = e.device_ptr(_lib.BUF_H)
        e.kl_step(1, shape.K)
        p1g = e.device_ptr(_lib.BUF_H)
        e.kl_step(1)
        p2 = e.device_ptr(_lib.BUF_H)
    finally:
        e.close()
    assert p0 and p1 and p2
    if shape.form == "paired":
        assert p1 != p0 and p1g == p1 and p2 == p0, (hex(p0), hex(p1), hex(p1g), hex(p2))
    else:
        assert p0 == p1 == p1g == p2, (hex(p0), hex(p1), hex(p1g), hex(p2))


REFUSALS = {
    # prefix, then these ops, then kl_rollback() is refused
    "P6q": ("P6q", []),
    "P6c": ("P6c", []),
    "P7": ("P7", []),
    "P4-second-rollback": ("P4", []),
    # MvNMF's speculation overwrites the buffer that holds the kept state: the state is given up, not handed back clobbered
    "P3-mv_step-queued": ("P3", [("set_mv_queued", True), ("mv_step", 1)]),
    "P3-mv_step-classic": ("P3", [("set_mv_queued", False), ("mv_step", 1)]),
    "P3-mv_step_objective-ahead": ("P3", [("mv_step_objective", 1, True)]),
    "P3-upload_H": ("P3", [("upload_H",)]),
}


@pytest.mark.parametrize("which", list(REFUSALS))
@pytest.mark.parametrize("shape", [RR.PRIMARY, RR.CONTROL], ids=lambda s: s.id)
def test_rollback_without_a_kept_state_is_refused_and_changes_nothing(shape, which):
    prefix, more = REFUSALS[which]
    g = grid()
    inp = RR.inputs(shape, g)
    engines = [new_engine(inp), new_engine(inp)]
    try:
        for e in engines:
            run(e, RR.PREFIXES[prefix] + more, inp, checks=False)
        a, ref = engines
        with pytest.raises(RuntimeError, match=NO_KEPT_STATE):
            a.kl_rollback()
        assert np.array_equal(a.download_W(), ref.download_W()) and np.array_equal(a.download_H(), ref.download_H()), "the refused call moved the state"
        # ... and the engine goes on as its twin does
        a.kl_step(1), ref.kl_step(1)
        assert np.array_equal(a.download_W(), ref.download_W()) and np.array_equal(a.download_H(), ref.download_H())
    finally:
        for e in engines:
            e.close()
