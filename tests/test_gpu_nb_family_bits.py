"""The negative-binomial entry points compute the recorded bits (``tests/golden/nb_family_bits.npz``).

``nb_refit_exposures``, ``draw_nb_counts``, ``nb_goodness_of_fit`` and ``estimate_dispersion`` run through the same host
drivers as their Poisson counterparts (``csrc/salnmf_refit_drivers.h``), which ``tests/test_gpu_refit_family_bits.py`` pins.
This is the same pin for the negative-binomial side: the record was written by ``tools/record_nb_bits.py`` on the build
before the drivers were shared, when each side still had a driver of its own.  Every case runs the four entry points at 37
samples -- three tiles, the last ragged -- with one signature count per instantiation of ``nb_refit_kernel`` (KT = 1 .. 6),
three chunks of resamples and of null draws, and per-sample dispersions below 1, around 20 and near 1e6.  Arrays of more
than ``FULL`` entries are compared by the SHA-256 of their dtype, shape and bytes (equal digests are equal bits)."""

import importlib.util
import os

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
_spec = importlib.util.spec_from_file_location("record_nb_bits", os.path.join(ROOT, "tools", "record_nb_bits.py"))
tool = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(tool)

with np.load(tool.GOLDEN) as fh:
    RECORD = {name: fh[name] for name in fh.files}


def test_the_record_covers_every_case_and_entry_point_and_nothing_else():
    assert np.array_equal(RECORD["seeds"], [tool.case_seed(c) for c in tool.CASES])
    heads = {tuple(name.split("/")[:2]) for name in RECORD if name != "seeds"}
    assert heads == {(tool.case_name(c), e) for c in tool.CASES for e in tool.ENTRIES}


@pytest.mark.parametrize("case", tool.CASES, ids=tool.case_name)
def test_nb_family_computes_the_recorded_bits(case):
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
