"""Development aid: nb_signature_presence_test against the composition it replaces, by device events.  Prints one JSON line.

The PCAWG breast catalogue (192 x 96) against the consensus signatures of a KLNMFSweep at K = 8, S = 3 tested signatures
(0, 1, 2), --draws B (default 200), alpha = 20 for every sample, default convergence settings, --repeats calls after a warm-up.
(a) nb_presence_kernel: the device-event time of the call's solve launches (1 + n_chunks of them), per repeat;
(b) the yardstick: the same solves by the negative-binomial assignment kernel -- per tested signature two masked
    nb_assign_signatures calls (candidates = required = the set, with and without s) on the call's own kept draws, and the same
    two on the counts --, the sum of their device-event times (assign_kernel_ms), per repeat.  2 S (1 + 1) launches;
(c) for context, signature_presence_test on the same input (its own draws: another model, another workload), same events.
The sums of iterations separate the model's cost (how long the solves run) from the step's."""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np
import pandas as pd

import salamander_amd as sal

ap = argparse.ArgumentParser()
ap.add_argument("--draws", type=int, default=200)
ap.add_argument("--repeats", type=int, default=5)
args = ap.parse_args()
B, TEST, SEED, ALPHA = args.draws, [0, 1, 2], 2024, 20.0

df = pd.read_csv(os.path.join(ROOT, "tests", "golden", "pcawg_breast_sbs.csv"), index_col=0)
X = np.ascontiguousarray(df.T.values, dtype=np.float64)
adata = sal.AnnData(X.copy())
adata.var_names = list(df.index)
K = 8
sweep = sal.models.KLNMFSweep(ns_signatures=[K], seeds=[0, 1, 2], stability=True, min_iterations=200, max_iterations=400)
sweep.fit(adata)
S = np.asarray(sweep.consensus_signatures_[0], dtype=np.float64)
S = S / S.sum(axis=1, keepdims=True)
N, V = X.shape


def spread(values):
    return {"median": round(float(np.median(values)), 3), "min": round(float(np.min(values)), 3), "max": round(float(np.max(values)), 3)}


def yardstick(res):
    """The negative-binomial assignment kernel's device-event time for the same solves: milliseconds, launches, iterations."""
    ms, launches, iterations = 0.0, 0, 0
    for j, s in enumerate(TEST):
        C = np.ones(K, dtype=bool)
        C0 = C.copy()
        C0[s] = False
        drawn = res.draws[:, :, j].reshape(B * N, V)
        for rows in (X, drawn):
            for A in (C, C0):
                fit = sal.nb_assign_signatures(rows, S, ALPHA, candidates=A, required=A)
                ms += fit.timings["assign_kernel_ms"]
                iterations += int(fit.n_iterations.sum())
                launches += 1
    return ms, launches, iterations


sal.nb_signature_presence_test(X[:32], S, ALPHA, TEST, n_draws=2, seed=1)  # warm-up: the code paths of the timed windows
sal.nb_assign_signatures(X[:32], S, ALPHA, candidates=np.ones(K, dtype=bool), required=np.ones(K, dtype=bool))
sal.signature_presence_test(X[:32], S, TEST, n_draws=2, seed=1)
mine, theirs, poisson, walls = [], [], [], []
for _ in range(args.repeats):
    t0 = time.perf_counter()
    res = sal.nb_signature_presence_test(X, S, ALPHA, TEST, n_draws=B, seed=SEED, keep_draws=True)
    walls.append(time.perf_counter() - t0)
    mine.append(res.timings["presence_kernel_ms"])
    ms, launches, yard_iterations = yardstick(res)
    theirs.append(ms)
    pres = sal.signature_presence_test(X, S, TEST, n_draws=B, seed=SEED)
    poisson.append(pres.timings["presence_kernel_ms"])
t = res.timings
print(json.dumps({
    "data": [N, V], "n_signatures": K, "test": TEST, "n_draws": B, "dispersion": ALPHA, "repeats": args.repeats,
    "nb_presence_kernel_ms": spread(mine), "presence_launches": 1 + t["n_chunks"], "draw_ms": round(t["draw_s"] * 1e3, 3),
    "reduce_ms": round(t["reduce_s"] * 1e3, 4), "wall_s": spread(walls), "nb_assign_kernel_ms": spread(theirs), "assign_launches": launches,
    "ratio_assign_over_presence": round(float(np.median(theirs) / np.median(mine)), 3),
    "solve_iterations": int(res.n_iterations.sum()) + int(res.null_n_iterations.sum()), "yardstick_iterations": yard_iterations,
    "poisson_presence_kernel_ms": spread(poisson), "poisson_solve_iterations": int(pres.n_iterations.sum()) + int(pres.null_n_iterations.sum()),
    "p_below_0.05": [int(v) for v in (res.p_value <= 0.05).sum(axis=0)], "poisson_p_below_0.05": [int(v) for v in (pres.p_value <= 0.05).sum(axis=0)],
}), flush=True)
