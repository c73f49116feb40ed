"""Development aid: exposure_change_test against the composition it replaces, by device events.  Prints one JSON line.

  --shape pcawg      the two halves of every sample of the PCAWG breast catalogue (192 x 96) by split_counts(train_fraction=0.5) --
                     null pairs by construction -- against the consensus signatures of a KLNMFSweep at K = 8
  --shape synthetic  --samples N (default 10 000) Poisson pairs of a Dirichlet catalogue at K = 64, b at a quarter of a's total
--draws B (default 200), default convergence settings, --repeats calls after a warm-up.
(a) change_kernel: the device-event time of the call's solve launches (1 + n_chunks of them), per repeat; the draw launches and
    the reduction beside it, and the wall time of the call;
(b) the yardstick: the same solves by the assignment kernel -- three masked assign_signatures calls (candidates = required =
    every signature: row a, row b, the sum of the clipped rows) on the counts and three on the call's own kept draws --, the sum
    of their device-event times (assign_kernel_ms), per repeat.  6 launches; the null divergences are not in it."""
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
B, SEED = args.draws, 2024
EPSILON = float(np.finfo(np.float32).eps)

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
    train, test = sal.split_counts(X, n_splits=1, train_fraction=0.5, seed=SEED)
    Xa, Xb = np.ascontiguousarray(train[0]), np.ascontiguousarray(test[0])
else:
    rng = np.random.default_rng(7)
    K = 64
    S = rng.dirichlet(np.full(96, 0.15), size=K)
    E = rng.dirichlet(np.full(K, 0.3), size=args.samples) * rng.uniform(200, 20000, size=(args.samples, 1))
    Xa, Xb = rng.poisson(E @ S).astype(np.float64), rng.poisson(0.25 * E @ S).astype(np.float64)
S = S / S.sum(axis=1, keepdims=True)
N, V = Xa.shape
ALL = np.ones(K, dtype=bool)


def spread(values):
    return {"median": round(float(np.median(values)), 3), "min": round(float(np.min(values)), 3), "max": round(float(np.max(values)), 3)}


def three_solves(A, Bm):
    """The assignment kernel's device-event time for the three solves of the rows (A, Bm): milliseconds, launches."""
    rows = (A, Bm, np.maximum(A, EPSILON) + np.maximum(Bm, EPSILON))
    return sum(sal.assign_signatures(r, S, candidates=ALL, required=ALL).timings["assign_kernel_ms"] for r in rows), 3


def yardstick(res):
    live = np.flatnonzero(res.tested)
    ms0, n0 = three_solves(Xa[live], Xb[live])
    drawn = res.draws[:, live]
    ms1, n1 = three_solves(drawn[:, :, 0].reshape(-1, V), drawn[:, :, 1].reshape(-1, V))
    return ms0 + ms1, n0 + n1


sal.exposure_change_test(Xa[:32], Xb[:32], S, n_draws=2, seed=1)  # warm-up: the code paths of the timed windows
sal.assign_signatures(Xa[:32], S, candidates=ALL, required=ALL)
mine, theirs, walls, draw_ms, reduce_ms = [], [], [], [], []
for _ in range(args.repeats):
    t0 = time.perf_counter()
    res = sal.exposure_change_test(Xa, Xb, S, n_draws=B, seed=SEED, keep_draws=True)
    walls.append(time.perf_counter() - t0)
    mine.append(res.timings["change_kernel_ms"])
    draw_ms.append(res.timings["draw_s"] * 1e3)
    reduce_ms.append(res.timings["reduce_s"] * 1e3)
    ms, launches = yardstick(res)
    theirs.append(ms)
t = res.timings
print(json.dumps({
    "shape": args.shape, "data": [N, V], "n_signatures": K, "n_draws": B, "repeats": args.repeats, "tested_pairs": int(res.tested.sum()),
    "change_kernel_ms": spread(mine), "change_launches": 1 + t["n_chunks"], "draw_ms": spread(draw_ms), "reduce_ms": spread(reduce_ms),
    "wall_s": spread(walls), "assign_kernel_ms": spread(theirs), "assign_launches": launches,
    "ratio_assign_over_change": round(float(np.median(theirs) / np.median(mine)), 3),
    "solve_iterations": int(res.n_iterations.sum()) + int(res.null_n_iterations.sum()), "p_below_0.05": int((res.p_value <= 0.05).sum()),
}), flush=True)
