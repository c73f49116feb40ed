"""Development aid: signature_change_test by device events, with exposure_change_test's solve rate on the same pairs as the
only yardstick (there is no earlier implementation, and no composition gives the tied solve).  Prints one JSON line.

  --shape pcawg      the two halves of every sample of the PCAWG breast catalogue (192 x 96) by split_counts(train_fraction=0.5) --
                     null pairs by construction -- against the consensus signatures of a KLNMFSweep at K = 8, every signature tested
  --shape synthetic  --samples N (default 2 000) Poisson pairs of a Dirichlet catalogue at K = 64, b at a quarter of a's total,
                     signatures 0, 31 and 63 tested
--draws B (default 200), default convergence settings, --repeats calls after a warm-up.
(a) sigchange_kernel: the device-event time of the call's solve launches (1 + n_chunks of them), per repeat; the draw launches
    and the reduction beside it, and the wall time of the call; the solve iterations (two free solves count their own, the tied
    solve twice: two columns step) over that time;
(b) the yardstick: change_kernel's column iterations per second on the same pairs in the same session."""
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
ap.add_argument("--samples", type=int, default=2000)
ap.add_argument("--draws", type=int, default=200)
ap.add_argument("--repeats", type=int, default=5)
args = ap.parse_args()
B, SEED = args.draws, 2024

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
    TEST = list(range(K))
else:
    rng = np.random.default_rng(7)
    K = 64
    S = rng.dirichlet(np.full(96, 0.15), size=K)
    E = rng.dirichlet(np.full(K, 0.3), size=args.samples) * rng.uniform(200, 20000, size=(args.samples, 1))
    Xa, Xb = rng.poisson(E @ S).astype(np.float64), rng.poisson(0.25 * E @ S).astype(np.float64)
    TEST = [0, 31, 63]
S = S / S.sum(axis=1, keepdims=True)
N, V = Xa.shape


def spread(values):
    return {"median": round(float(np.median(values)), 3), "min": round(float(np.min(values)), 3), "max": round(float(np.max(values)), 3)}


def column_iterations(res, tied_twice):
    """Steps of lane columns in a call's solves: every solve's own count, the tied solve's twice (it steps two columns)."""
    total = 0
    for nit in (res.n_iterations, res.null_n_iterations):
        nit = nit.astype(np.int64)
        total += int(nit.sum()) + (int(nit[..., 2].sum()) if tied_twice else 0)
    return total


sal.signature_change_test(Xa[:32], Xb[:32], S, TEST[:1], n_draws=2, seed=1)  # warm-up: the code paths of the timed windows
sal.exposure_change_test(Xa[:32], Xb[:32], S, n_draws=2, seed=1)
mine, walls, draw_ms, reduce_ms, theirs = [], [], [], [], []
for _ in range(args.repeats):
    t0 = time.perf_counter()
    res = sal.signature_change_test(Xa, Xb, S, TEST, n_draws=B, seed=SEED)
    walls.append(time.perf_counter() - t0)
    mine.append(res.timings["sigchange_kernel_ms"])
    draw_ms.append(res.timings["draw_s"] * 1e3)
    reduce_ms.append(res.timings["reduce_s"] * 1e3)
    other = sal.exposure_change_test(Xa, Xb, S, n_draws=B, seed=SEED)
    theirs.append(other.timings["change_kernel_ms"])
its, its_other = column_iterations(res, True), column_iterations(other, False)
rate, rate_other = its / (np.median(mine) * 1e-3), its_other / (np.median(theirs) * 1e-3)
t = res.timings
print(json.dumps({
    "shape": args.shape, "data": [N, V], "n_signatures": K, "n_test": len(TEST), "n_draws": B, "repeats": args.repeats,
    "tested_problems": int(res.tested.sum()), "sigchange_kernel_ms": spread(mine), "sigchange_launches": 1 + t["n_chunks"], "draw_ms": spread(draw_ms),
    "reduce_ms": spread(reduce_ms), "wall_s": spread(walls), "column_iterations": its, "column_iterations_per_s": round(rate),
    "change_kernel_ms": spread(theirs), "change_column_iterations": its_other, "change_column_iterations_per_s": round(rate_other),
    "rate_over_change_kernel": round(float(rate / rate_other), 3), "p_below_0.05": int((res.p_value <= 0.05).sum()),
}), flush=True)
