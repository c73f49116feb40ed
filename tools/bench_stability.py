"""Development aid: what ``KLNMFSweep(stability=True)`` adds to a bootstrap sweep, on the PCAWG breast catalogue (192 x 96)
with the settings of tools/bench_bootstrap.py: K = 1..16, one seed, init_method="random", default convergence settings, for
R = 8 and R = 100 resamples.  Prints one JSON line (profiles/sweep/bench_stability.json) with, per R:
(a) the sweep's wall time with stability=False and with stability=True (each the second of two runs) and timings_["stability_s"];
(b) the stability kernel alone by device events, on the same signatures in the stand-alone form (all 16 groups in one launch;
    every one of 5 calls is listed);
(c) the host replica (tests/_stability_ref.py: NumPy + SciPy's linear_sum_assignment, without its margin re-solves) on the same
    signatures -- the yardstick: the kernel is not compared with itself -- and whether both give the same assignments."""
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import numpy as np
import pandas as pd

import _stability_ref as ref
import salamander_amd as sal

df = pd.read_csv(os.path.join(ROOT, "tests", "golden", "pcawg_breast_sbs.csv"), index_col=0)
X = np.ascontiguousarray(df.T.values, dtype=np.float64)
adata = sal.AnnData(X.copy())
KS, SEED = list(range(1, 17)), 2024


def sweep(R, stability):
    s = sal.models.KLNMFSweep(KS, seeds=[0], init_method="random", n_resamples=R, resample_seed=SEED, stability=stability)
    t0 = time.perf_counter()
    s.fit(adata)
    return s, time.perf_counter() - t0


def measure(R):
    sweep(R, False)
    _, plain_s = sweep(R, False)
    sweep(R, True)
    s, with_s = sweep(R, True)
    groups = [np.stack([np.asarray(m.asignatures.X) for m in s.models_[g * R : (g + 1) * R]]) for g in range(len(KS))]
    errors = [[m.reconstruction_error for m in s.models_[g * R : (g + 1) * R]] for g in range(len(KS))]
    kernel_ms, calls_s = [], []
    for _ in range(5):
        t0 = time.perf_counter()
        got = sal.signature_stability(groups, errors)
        calls_s.append(round(time.perf_counter() - t0, 5))
        kernel_ms.append(round(got[0].kernel_ms, 4))
    t0 = time.perf_counter()
    want = [ref.stability(g, e, margins=False) for g, e in zip(groups, errors)]
    replica_s = time.perf_counter() - t0
    return {
        "n_resamples": R, "members": len(s.models_), "all_batched": bool(s.batched_.all()),
        "sweep_s": round(plain_s, 4), "sweep_with_stability_s": round(with_s, 4), "stability_s": round(s.timings_["stability_s"], 5),
        "batched_s": round(s.timings_["batched_s"], 4), "init_s": round(s.timings_["init_s"], 4),
        "kernel_ms_by_events": kernel_ms, "stand_alone_call_s": calls_s, "replica_s": round(replica_s, 5),
        "rounds": [int(r) for r in s.stability_rounds_], "converged": [bool(c) for c in s.stability_converged_],
        "same_assignments_as_replica": [bool(np.array_equal(a.assignments, b.assignments)) for a, b in zip(got, want)],
        "stability_mean": [round(float(v), 4) for v in s.stability_mean_], "stability_min": [round(float(v), 4) for v in s.stability_min_],
        "suggested": s.suggest_n_signatures(),
    }


out = {"data": list(X.shape), "ns_signatures": [KS[0], KS[-1]], "runs": [measure(8), measure(100)]}
print(json.dumps(out), flush=True)
