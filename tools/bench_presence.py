"""Development aid: signature_presence_test against the composition it replaces, by device events.  Prints one JSON line.

  --shape pcawg      the PCAWG breast catalogue (192 x 96) against the consensus signatures of a KLNMFSweep at K = 8
  --shape synthetic  --samples N (default 10 000) Poisson samples of a Dirichlet catalogue at K = 64
S = 3 tested signatures (0, 1, 2), --draws B (default 200), default convergence settings, --repeats calls after a warm-up.
(a) presence_kernel: the device-event time of the call's solve launches (1 + n_chunks of them), per repeat;
(b) the yardstick: the same solves by the assignment kernel -- per tested signature two masked assign_signatures calls
    (candidates = required = the set, with and without s) on the call's own kept draws, and the same two on the counts --, the
    sum of their device-event times (assign_kernel_ms), per repeat.  2 S (1 + 1) launches."""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np

import salamander_amd as sal

ap = argparse.ArgumentParser()
ap.add_argument("--shape", choices=("pcawg", "synthetic"), default="pcawg")
ap.add_argument("--samples", type=int, default=10000)
ap.add_argument("--draws", type=int, default=200)
ap.add_argument("--repeats", type=int, default=5)
args = ap.parse_args()
B, TEST, SEED = args.draws, [0, 1, 2], 2024

if args.shape == "pcawg":
    import pandas as pd

    df = pd.read_csv(os.path.join(ROOT, "tests", "golden", "pcawg_breast_sbs.csv"), index_col=0)
    X = np.ascontiguousarray(df.T.values, dtype=np.float64)
    adata = sal.AnnData(X.copy())
    adata.var_names = list(df.index)
    K = 8
    sweep = sal.models.KLNMFSweep(ns_signatures=[K], seeds=[0, 1, 2], stability=True, min_iterations=200, max_iterations=400)
    sweep.fit(adata)
    S = np.asarray(sweep.consensus_signatures_[0], dtype=np.float64)
else:
    rng = np.random.default_rng(7)
    K = 64
    S = rng.dirichlet(np.full(96, 0.15), size=K)
    E = rng.dirichlet(np.full(K, 0.3), size=args.samples) * rng.uniform(200, 20000, size=(args.samples, 1))
    X = rng.poisson(E @ S).astype(np.float64)
S = S / S.sum(axis=1, keepdims=True)
N, V = X.shape


def spread(values):
    return {"median": round(float(np.median(values)), 3), "min": round(float(np.min(values)), 3), "max": round(float(np.max(values)), 3)}


def yardstick(res):
    """The assignment kernel's device-event time for the same solves: milliseconds, launches."""
    ms, launches = 0.0, 0
    for j, s in enumerate(TEST):
        C = np.ones(K, dtype=bool)
        C0 = C.copy()
        C0[s] = False
        drawn = res.draws[:, :, j].reshape(B * N, V)
        for rows in (X, drawn):
            for A in (C, C0):
                ms += sal.assign_signatures(rows, S, candidates=A, required=A).timings["assign_kernel_ms"]
                launches += 1
    return ms, launches


sal.signature_presence_test(X[:32], S, TEST, n_draws=2, seed=1)  # warm-up: the code paths of the timed windows
sal.assign_signatures(X[:32], S, candidates=np.ones(K, dtype=bool), required=np.ones(K, dtype=bool))
mine, theirs, walls = [], [], []
for _ in range(args.repeats):
    t0 = time.perf_counter()
    res = sal.signature_presence_test(X, S, TEST, n_draws=B, seed=SEED, keep_draws=True)
    walls.append(time.perf_counter() - t0)
    mine.append(res.timings["presence_kernel_ms"])
    ms, launches = yardstick(res)
    theirs.append(ms)
t = res.timings
print(json.dumps({
    "shape": args.shape, "data": [N, V], "n_signatures": K, "test": TEST, "n_draws": B, "repeats": args.repeats,
    "presence_kernel_ms": spread(mine), "presence_launches": 1 + t["n_chunks"], "draw_ms": round(t["draw_s"] * 1e3, 3),
    "reduce_ms": round(t["reduce_s"] * 1e3, 4), "wall_s": spread(walls), "assign_kernel_ms": spread(theirs), "assign_launches": launches,
    "ratio_assign_over_presence": round(float(np.median(theirs) / np.median(mine)), 3),
    "solve_iterations": int(res.n_iterations.sum()) + int(res.null_n_iterations.sum()), "p_below_0.05": [int(v) for v in (res.p_value <= 0.05).sum(axis=0)],
}), flush=True)
