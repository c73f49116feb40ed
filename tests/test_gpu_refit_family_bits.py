"""The refit family computes the recorded bits (``tests/golden/refit_family_bits.npz``).

``refit_exposures``, ``assign_signatures`` (plain, and with candidates, required signatures and the re-addition pass),
``goodness_of_fit``, ``signature_presence_test``, ``signature_power``, ``profile_likelihood`` and ``exposure_intervals`` are
built from one set of kernel pieces (``csrc/salnmf_refit.h``) and one host kit (``csrc/salnmf_refit.hip``).  A problem's result
depends on its row and the signatures alone and every sum has a fixed order, so a build gives the same bits on every run, and
the pieces and the kit can be rearranged without changing any of them as long as every kernel keeps its operations in their
order and every call issues the launches it issued before.  The record was written by ``tools/record_refit_bits.py`` on a
build whose kernels and drivers did not yet use the shared pieces and kit.  Every case runs the seven entry points (the
assignment twice: plain, and with candidates, required signatures and the re-addition pass) at 37
samples -- three tiles, the last ragged -- with one signature count per kernel instantiation (KT = 1 .. 6), three chunks of
resamples, null draws and alternative draws, untested pairs, a profile that spans two runs of values, and a tolerance at
which some columns stop early and others do not.  The cases ``FULL_CASES`` hold every array in full; in the others arrays of more than
``FULL`` entries are compared by the SHA-256 of their dtype, shape and bytes (equal digests are equal bits)."""

import importlib.util
import os

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
_spec = importlib.util.spec_from_file_location("record_refit_bits", os.path.join(ROOT, "tools", "record_refit_bits.py"))
tool = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(tool)

with np.load(tool.GOLDEN) as fh:
    RECORD = {name: fh[name] for name in fh.files}


def test_the_record_covers_every_case_and_entry_point_and_nothing_else():
    assert np.array_equal(RECORD["seeds"], [tool.case_seed(c) for c in tool.CASES])
    heads = {tuple(name.split("/")[:2]) for name in RECORD if name != "seeds"}
    assert heads == {(tool.case_name(c), e) for c in tool.CASES for e in tool.ENTRIES}


@pytest.mark.parametrize("case", tool.CASES, ids=tool.case_name)
def test_refit_family_computes_the_recorded_bits(case):
    prefix = tool.case_name(case) + "/"
    got = {prefix + name: a for name, a in tool.run_case(case).items()}
    want = {name: a for name, a in RECORD.items() if name.startswith(prefix)}
    assert sorted(got) == sorted(want)  # the same arrays, name by name
    for name in sorted(want):
        assert got[name].dtype == want[name].dtype and got[name].shape == want[name].shape, name
    differing = {}
    for name in sorted(want):
        g, w = got[name], want[name]
        if not np.array_equal(g, w, equal_nan=g.dtype.kind == "f"):
            bad = ~((g == w) | ((g != g) & (w != w)) if g.dtype.kind == "f" else (g == w))
            first = tuple(int(i) for i in np.argwhere(bad)[0])
            differing[name] = f"{int(bad.sum())} of {g.size} entries differ, first at {first}: {g[first]!r} != {w[first]!r}"
    assert not differing, differing
