"""Record what the negative-binomial entry points compute, bit for bit: ``nb_refit_exposures``, ``draw_nb_counts``,
``nb_goodness_of_fit`` and ``estimate_dispersion``.

The companion of ``tools/record_refit_bits.py`` (whose hash, inputs, case names and digests this tool imports) for the
negative-binomial side of the refit family: ``tests/test_gpu_nb_family_bits.py`` compares with
``tests/golden/nb_family_bits.npz``, written by

    python tools/record_nb_bits.py [path of the record]

on a build known to be right (run it twice: the two records must be identical).  The kernels use fixed-order sums, a
problem's result depends on its row, its dispersion and the signatures alone, and the draws are counter-based, so a build
computes the same record on every run, and a change that moves host code without changing a launch computes the same record
as the build before it.

Shapes: 37 samples (three tiles of 16, the last ragged); one signature count per instantiation of ``nb_refit_kernel``
(KT = 1 .. 6), the feature axis full (96) and ragged (83).  Every sample has its own dispersion, in turn below 1, around 20 and
near 1e6, so that every tile holds all three and both shape branches of the gamma draw occur.  The record holds every array an
entry point returns and the counts its ``timings`` carry (never the milliseconds): an array of at most ``FULL`` entries as it
is, a larger one as its SHA-256.
"""
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
import numpy as np
from record_refit_bits import ITER, TOL, B, N, case_name, case_seed, encode, flatten, inputs, uniform

GOLDEN = os.path.join(ROOT, "tests", "golden", "nb_family_bits.npz")

CASES = [(96, 5), (83, 17), (96, 40), (96, 50), (96, 70), (83, 96)]  # (V, K)
GRID = (0.5, 20.0, 1e5)
ENTRIES = ("nb_refit", "nb_draw", "nb_gof", "dispersion")


def dispersions(case):
    """(N,) dispersions: samples 0, 3, .. in [0.3, 0.9), samples 1, 4, .. in [15, 25), samples 2, 5, .. in [9e5, 1e6)."""
    u = uniform(case_seed(case) + 10, N)
    return np.choose(np.arange(N) % 3, [0.3 + 0.6 * u, 15.0 + 10.0 * u, 1e6 * (0.9 + 0.1 * u)])


def run_case(case):
    """name -> array (or digest) of everything the four calls of one case return."""
    from salamander_amd.nb import draw_nb_counts, estimate_dispersion, nb_goodness_of_fit, nb_refit_exposures

    V, K = case
    X, W = inputs(case)[:2]
    alpha = dispersions(case)
    assert (alpha < 1.0).any() and (alpha >= 1.0).any()  # both shape branches of the gamma draw
    it = dict(ITER, tol=TOL[K])
    rows = 2 * N * V * 8  # two resamples (draws) per chunk: three chunks for five
    refit = nb_refit_exposures(X, W, alpha, n_resamples=B, resample_seed=21, keep_resamples=True, chunk_bytes=rows, **it)
    gof = nb_goodness_of_fit(X, W, alpha, n_draws=B, seed=23, keep_draws=True, chunk_bytes=rows, **it)
    assert refit.timings["n_chunks"] == 3 and gof.timings["n_chunks"] == 3, (refit.timings, gof.timings)
    arrays = {"nb_draw/draws": draw_nb_counts(refit.exposures, W, alpha, B, seed=22)}
    flatten("nb_refit", refit, arrays)
    flatten("nb_gof", gof, arrays)
    flatten("dispersion", estimate_dispersion(X, W, np.array(GRID), per_sample=True, **it), arrays)
    assert {name.split("/")[0] for name in arrays} == set(ENTRIES)
    return encode(arrays)


def record():
    out = {"seeds": np.array([case_seed(c) for c in CASES], dtype=np.int64)}
    for case in CASES:
        for name, a in run_case(case).items():
            out[f"{case_name(case)}/{name}"] = a
    return out


if __name__ == "__main__":
    path = sys.argv[1] if len(sys.argv) > 1 else GOLDEN
    rec = record()
    np.savez_compressed(path, **rec)
    print(f"{len(CASES)} cases, {len(rec)} entries, {os.path.getsize(path)} bytes -> {path}")
    assert os.path.getsize(path) < (1 << 20), "the record must stay below 1 MiB"
