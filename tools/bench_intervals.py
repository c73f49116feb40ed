"""Development aid: exposure_intervals on the PCAWG breast catalogue, by device events.  Prints one JSON line and, with --out,
writes it to a file (profiles/intervals/bench_intervals_pcawg.json).

The catalogue (192 x 96) against the consensus signatures of a KLNMFSweep at K = 10; every signature is tested in every sample,
at the default threshold, search and convergence settings; --repeats calls after a warm-up.  Times as measured: the observed
launch (the presence kernel's), the one profile_kernel launch, and the wall time of the call.  There is no earlier
implementation to compare with."""
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
ap.add_argument("--signatures", type=int, default=10)
ap.add_argument("--repeats", type=int, default=5)
ap.add_argument("--out", default=None)
args = ap.parse_args()
K = args.signatures
TEST = list(range(K))

df = pd.read_csv(os.path.join(ROOT, "tests", "golden", "pcawg_breast_sbs.csv"), index_col=0)
X = np.ascontiguousarray(df.T.values, dtype=np.float64)
adata = sal.AnnData(X.copy())
adata.var_names = list(df.index)
sweep = sal.models.KLNMFSweep(ns_signatures=[K], seeds=[0, 1, 2], stability=True, min_iterations=200, max_iterations=400)
sweep.fit(adata)
S = np.asarray(sweep.consensus_signatures_[0], dtype=np.float64)
S = S / S.sum(axis=1, keepdims=True)
N, V = X.shape


def spread(values):
    return {"median": round(float(np.median(values)), 3), "min": round(float(np.min(values)), 3), "max": round(float(np.max(values)), 3)}


sal.exposure_intervals(X[:32], S, TEST[:2], n_bisections=2)  # warm-up: the code paths of the timed windows
observed, profile, walls = [], [], []
for _ in range(args.repeats):
    t0 = time.perf_counter()
    res = sal.exposure_intervals(X, S, TEST)
    walls.append(time.perf_counter() - t0)
    observed.append(res.timings["observed_kernel_ms"])
    profile.append(res.timings["profile_kernel_ms"])
t = res.tested
width = (res.upper - res.lower)[t & res.bracketed]
line = {
    "shape": "pcawg", "data": [N, V], "n_signatures": K, "test": TEST, "max_kl_increase": res.max_kl_increase, "n_bisections": 16, "max_expansions": 40,
    "repeats": args.repeats, "pairs": int(t.sum()), "problems": res.timings["n_problems"], "trials": int(res.n_trials.sum()),
    "trials_per_end": {"lower_max": int(res.n_trials[..., 0].max()), "upper_max": int(res.n_trials[..., 1].max())},
    "observed_kernel_ms": spread(observed), "profile_kernel_ms": spread(profile), "wall_s": spread(walls),
    "lower_is_zero": int((res.lower[t] == 0.0).sum()), "unbracketed": int((~res.bracketed[t]).sum()), "median_width": round(float(np.median(width)), 3),
}
print(json.dumps(line), flush=True)
if args.out:
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as fh:
        fh.write(json.dumps(line, indent=1) + "\n")
