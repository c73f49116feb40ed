"""The tables of ``tests/_rotation_ref.py`` are not vacuous (no GPU): every public ``Engine`` method is classified, every
shape has the form its row claims on three grids, and no oracle reference could be met by a probe that did nothing or read
the state of one step earlier."""

import inspect

import numpy as np
import pytest

import _rotation_ref as RR
from salamander_amd.engine import Engine

G_HOST = 64  # the references below are formed on a 64-workgroup grid: a quarter of the samples, the same code


def test_every_public_engine_method_is_classified():
    public = {n for n, f in inspect.getmembers(Engine, predicate=lambda o: inspect.isfunction(o) or isinstance(o, staticmethod)) if not n.startswith("_")}
    public |= {n for n, f in vars(Engine).items() if isinstance(f, staticmethod)}
    table, harness, exempt = RR.table_methods(), set(RR.HARNESS), set(RR.EXEMPT)
    assert table <= public, f"the tables name what Engine does not have: {sorted(table - public)}"
    assert harness <= public and exempt <= public, sorted((harness | exempt) - public)
    assert not (table & exempt), f"both a table entry and exempt: {sorted(table & exempt)}"
    missing = public - table - harness - exempt
    assert not missing, f"new entry points: put them into a prefix or a probe of tests/_rotation_ref.py, or exempt them with a reason: {sorted(missing)}"
    assert all(isinstance(r, str) and r for r in list(RR.EXEMPT.values()) + list(RR.HARNESS.values()))
    # what the issue lists as untested behind a swap is in the tables, not in the exemptions
    for name in ("update_H", "update_W", "mv_step", "mv_step_objective", "mv_objective", "mv_logdet", "set_H_scale", "kl_step_objective", "kl_step_partial",
                 "kl_step_finish", "set_precision", "set_weights", "upload_H", "corr_compute_exposures", "kl_step_keep", "kl_rollback", "set_persistent",
                 "objective", "samplewise_kl", "reconstruct"):
        assert name in table, name
    assert "device_ptr" in harness


@pytest.mark.parametrize("g", [64, 256, 304])
def test_every_shape_has_the_form_its_row_claims(g):
    for s in RR.SHAPES:
        L = RR.leftover(s.which, g)
        assert RR.form(L, g) == s.form, (s, g)
        N = RR.samples(s.which, g)
        tiles = (N + 15) // 16
        assert tiles == 4 * g + L and N % 16 != 0
        assert min(g, (tiles + 3) // 4) == g  # (salnmf_create: the engine's grid is g)
        assert (0 < 2 * (tiles % (4 * g)) <= g) == (s.form == "paired")  # salnmf.hip: leftover_pairs
        assert tiles > 64  # the one-workgroup kernel never takes the shape
    assert [s.form for s in RR.SHAPES].count("single") == 1 and RR.CONTROL.which == "half+1"


def test_the_case_list_is_the_cross_the_issue_asks_for():
    cases = RR.cases()
    assert len(set(map(RR.case_id, cases))) == len(cases)
    primary = [(p, q) for s, p, q in cases if s is RR.PRIMARY]
    assert sorted(primary) == sorted((p, q) for p in RR.PREFIXES for q in RR.PROBES)
    for s in RR.SHAPES:
        if s is RR.PRIMARY:
            continue
        mine = [(p, q) for t, p, q in cases if t is s]
        assert {p for p, q in mine if q == "kl_step2"} == set(RR.PREFIXES)
        assert {q for p, q in mine if p == "P1"} == set(RR.PROBES)
    assert len(RR.PREFIXES) == 15 and {"P6q", "P6c"} <= set(RR.PREFIXES)


def _share_changed(a, b, tol):
    return float(np.mean(np.abs(a - b) > tol * np.abs(b)))


@pytest.fixture(scope="module")
def p1():
    return RR.inputs(RR.PRIMARY, G_HOST), RR.prefix_state(RR.PRIMARY, G_HOST, "P1"), RR.prefix_state(RR.PRIMARY, G_HOST, "P2")


# which of (W, H) a probe rewrites, and the tolerance its result is held to
WRITES = {"kl_step1": "WH", "kl_step2": "WH", "keep_rollback": "WH", "step_objective": "WH", "update_H": "H", "update_W": "W", "mv_step": "WH",
          "mv_ahead_then_kl": "WH", "partial_finish": "WH", "f32_step": "WH", "weights_step": "WH", "corr": "WH"}
READS = {"objective": RR.OBJ_RTOL, "samplewise_kl": RR.SKL_RTOL, "reconstruct": RR.REC_RTOL, "mv_objective": RR.MV_OBJ_RTOL, "step_objective": RR.OBJ_RTOL}


@pytest.mark.parametrize("probe", list(RR.PROBES))
def test_no_reference_is_met_by_a_probe_that_did_nothing(p1, probe):
    inp, s1, s2 = p1
    assert set(WRITES) | set(READS) | {"mv_logdet"} == set(RR.PROBES)
    st, returned = RR.oracle_run(inp, s1, RR.PROBES[probe])
    tol = {"f64": RR.TOL, "mv": RR.MV_L2, "f32": max(RR.fr.bound_H(*s1.W.shape), RR.fr.bound_W(s1.W.shape[0], 2))}[st.kind]
    if "W" in WRITES.get(probe, ""):
        free = slice(2, None) if probe == "update_W" else slice(None)
        assert _share_changed(st.W[free], s1.W[free], tol) >= 0.5, probe
    if "H" in WRITES.get(probe, ""):
        assert _share_changed(st.H, s1.H, tol) >= 0.5, probe
    if probe not in WRITES:
        assert st.W is s1.W and st.H is s1.H
    # a reader that saw the state of one step earlier or later (a stale pointer) is far outside the tolerance
    if probe in READS:
        other = RR.oracle_run(inp, s2, RR.PROBES[probe])[1]
        a, b = np.asarray(returned[0].value), np.asarray(other[0].value)
        assert np.mean(np.abs(a - b) > 100 * READS[probe] * np.abs(a)) >= 0.5, probe
    if probe == "mv_logdet":  # reads W alone
        other = RR.oracle_run(inp, s2, RR.PROBES[probe])[1]
        assert abs(returned[0].value - other[0].value) > 100 * RR.MV_LOGDET_RTOL * abs(returned[0].value)
    if probe == "corr":
        Hc = returned[0].value
        Hld, unit = RR.corr_exposures_ld(RR.PRIMARY, G_HOST)
        assert _share_changed(Hc, s1.H, float(RR.R.C["H"] * np.max(unit))) >= 0.5
        assert RR.R.rel_ratio(Hc, Hld, unit)[0] <= RR.R.ORACLE_RATIO["H"]  # (the float64 oracle is within its own measured ratio)


def test_the_prefixes_leave_distinct_states(p1):
    """P0, P1, P2 differ pairwise (a rollback to the wrong buffer, or a reader of the buffer before the swap, is visible); P4
    and P5 return to P1's state; the scale of P8 puts a share of H on the floor and lifts a column."""
    inp, s1, s2 = p1
    s0 = RR.start_state(inp)
    for a, b in ((s0, s1), (s1, s2), (s0, s2)):
        assert _share_changed(a.H, b.H, RR.TOL) >= 0.5 and _share_changed(a.W, b.W, RR.TOL) >= 0.5
    for p in ("P4", "P5"):
        s = RR.prefix_state(RR.PRIMARY, G_HOST, p)
        assert np.array_equal(s.W, s1.W) and np.array_equal(s.H, s1.H) and s.kept is None
    s8 = RR.prefix_state(RR.PRIMARY, G_HOST, "P8")
    assert np.mean(s8.H == RR.orc.EPSILON) >= 0.05 and (s8.H > 1.5 * s1.H).all(axis=0).any()  # (_scale_ref: the share that clips)
    assert RR.prefix_state(RR.PRIMARY, G_HOST, "P3").kept is not None
    for p in ("P6q", "P6c", "P7"):
        s = RR.prefix_state(RR.PRIMARY, G_HOST, p)
        assert s.kept is None and s.kind == "mv"
        with pytest.raises(RuntimeError, match="no kept state"):
            RR.oracle_op(inp, s, ("kl_rollback",))
    assert RR.prefix_state(RR.PRIMARY, G_HOST, "P11").kind == "f32"
    s12 = RR.prefix_state(RR.PRIMARY, G_HOST, "P12")
    assert s12.H is inp.Hup and np.array_equal(s12.W, s1.W)
