"""Development aid: KLNMFSweep with bootstrap resamples against what a user could do without them, on the PCAWG breast
catalogue (192 x 96): K = 1..16 x R = 8 resamples, init_method="random", default convergence settings.  Prints one JSON line:
(a) the sweep's wall time, split into resample / init / batched loop;
(b) the baseline: the same 128 resample-fits with the resamples drawn on the host (numpy.random.default_rng(seed).multinomial
    per row) and KLNMF.fit(objective_in_step=False) one after another, in the same process after the same warm-up;
(c) the resample kernel alone by device events, in draws per second, against the host sampler's draws per second for the
    same 128 x 192 rows (R = 128: one matrix per member, what a bootstrap without pairing across K would draw)."""
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np
import pandas as pd

import salamander_amd as sal
from salamander_amd.batch import BatchEngine

df = pd.read_csv(os.path.join(ROOT, "tests", "golden", "pcawg_breast_sbs.csv"), index_col=0)
X = np.ascontiguousarray(df.T.values, dtype=np.float64)
adata = sal.AnnData(X.copy())
KS, R, SEED = list(range(1, 17)), 8, 2024
totals = X.sum(axis=1).astype(np.int64)
P = X / X.sum(axis=1, keepdims=True)


def host_resamples(n, seed):
    rng = np.random.default_rng(seed)
    return np.stack([np.stack([rng.multinomial(totals[i], P[i]) for i in range(len(X))]) for _ in range(n)]).astype(np.float64)


def sweep():
    s = sal.models.KLNMFSweep(KS, seeds=[0], init_method="random", n_resamples=R, resample_seed=SEED)
    t0 = time.perf_counter()
    models = s.fit(adata)
    wall = time.perf_counter() - t0
    t = s.timings_
    return {"members": len(models), "all_batched": bool(s.batched_.all()), "sweep_s": round(wall, 4), "resample_s": round(t["resample_s"], 4),
            "init_s": round(t["init_s"], 4), "batched_s": round(t["batched_s"], 4), "member_steps": int(sum(m.n_iterations_ for m in models))}


def baseline():
    t0 = time.perf_counter()
    mats = host_resamples(R, SEED)
    t_draw = time.perf_counter() - t0
    steps = 0
    for K in KS:
        for r in range(R):
            m = sal.models.KLNMF(K, "random", objective_in_step=False)
            m.fit(sal.AnnData(mats[r].copy()), init_kwargs={"seed": 0})
            steps += m.n_iterations_
            m._engine.close()
    return {"sequential_s": round(time.perf_counter() - t0, 4), "host_resample_s": round(t_draw, 4), "member_steps": int(steps)}


def kernel_alone(n_matrices=128, n_calls=20):
    draws = int(totals.sum()) * n_matrices
    b = BatchEngine(X.shape[0], X.shape[1], [1])
    try:
        b.upload_X(X, clip=True)
        ms = b.profile_resample(n_matrices, SEED, n_calls)
    finally:
        b.close()
    host_resamples(1, 1)
    t0 = time.perf_counter()
    host_resamples(n_matrices, SEED)
    host_s = time.perf_counter() - t0
    return {"matrices": n_matrices, "draws": draws, "kernel_ms": round(ms, 4), "kernel_draws_per_s": round(draws / (ms * 1e-3), 1),
            "host_s": round(host_s, 4), "host_draws_per_s": round(draws / host_s, 1), "factor": round(host_s / (ms * 1e-3), 1)}


# warm-up: every shape and code path of the timed windows
sal.models.KLNMFSweep([1, 5, 16], seeds=[0], init_method="random", min_iterations=20, max_iterations=20, n_resamples=2).fit(adata)
for K in (1, 5, 16):
    w = sal.models.KLNMF(K, "random", objective_in_step=False, min_iterations=20, max_iterations=20)
    w.fit(sal.AnnData(X.copy()), init_kwargs={"seed": 0})
    w._engine.close()
out = {"data": list(X.shape), "ns_signatures": [KS[0], KS[-1]], "n_resamples": R, "draws_per_resample": int(totals.sum())}
out["sweep"] = sweep()
out["sweep_again"] = sweep()
out["baseline"] = baseline()
out["speedup_wall"] = round(out["baseline"]["sequential_s"] / out["sweep_again"]["sweep_s"], 2)
out["resample_kernel"] = kernel_alone()
print(json.dumps(out), flush=True)
