"""Engines with feature blocks, signature chunks or both compute the recorded bits (``tests/golden/wide_bits.json``).

The update passes use no atomics and fixed-order two-stage sums, so one build gives the same bits on every
run, and the host logic that drives the (block, chunk) grid (``csrc/salnmf_host_wide.h``) can be changed without changing
any of them as long as every regime issues the launches it issued before.  The record was written by
``tools/record_wide_bits.py`` on the build before the three drivers (blocks, chunks, both) became one; its two runs there
were identical.  Each case is one script over every entry point that reaches the wide logic: objective, joint steps,
update_H, update_W, a kept block and its rollback, a step with a queued objective, samplewise_kl, reconstruct, MvNMF steps
and their objective -- and the CorrNMF aux / update_signatures pair on feature blocks."""

import importlib.util
import json
import os

import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
_spec = importlib.util.spec_from_file_location("record_wide_bits", os.path.join(ROOT, "tools", "record_wide_bits.py"))
tool = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(tool)

with open(tool.GOLDEN) as fh:
    RECORD = json.load(fh)


def test_the_record_covers_every_case_and_nothing_else():
    assert sorted(RECORD) == sorted(tool.case_name(c) for c in tool.CASES)


@pytest.mark.parametrize("case", tool.CASES, ids=tool.case_name)
def test_wide_engine_computes_the_recorded_bits(case):
    got, want = tool.run_case(case), RECORD[tool.case_name(case)]
    assert [g[0] for g in got] == [w[0] for w in want]  # the same script, entry by entry
    differing = [(g[0], g[1], w[1]) for g, w in zip(got, want) if g[1] != w[1]]
    assert not differing, differing
