"""Development aid: nb_assign_signatures next to assign_signatures on the PCAWG breast catalogue (192 x 96) against the consensus
signatures of a KLNMFSweep at K = 8, default convergence settings and threshold, without resamples and with R = 200.  The figure
is timings["assign_kernel_ms"], device events around the assignment launches; --repeats calls after a warm-up of the same shape,
median and range.  Prints one JSON line (profiles/nb_assign/ holds the recorded one).  --dispersion is the alpha of every sample."""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np
import pandas as pd

import salamander_amd as sal

ap = argparse.ArgumentParser()
ap.add_argument("--repeats", type=int, default=5)
ap.add_argument("--resamples", type=int, default=200)
ap.add_argument("--dispersion", type=float, default=20.0)
ap.add_argument("--signatures", type=int, default=8)
args = ap.parse_args()

df = pd.read_csv(os.path.join(ROOT, "tests", "golden", "pcawg_breast_sbs.csv"), index_col=0)
X = np.ascontiguousarray(df.T.values, dtype=np.float64)
K = args.signatures
sweep = sal.models.KLNMFSweep(ns_signatures=[K], seeds=[0, 1, 2], stability=True, min_iterations=200, max_iterations=400)
sweep.fit(sal.AnnData(X.copy()))
S = np.asarray(sweep.consensus_signatures_[0], dtype=np.float64)
S = S / S.sum(axis=1, keepdims=True)


def measure(call, R):
    call(R)  # warm-up: the same shape and code path
    ms = [call(R).timings["assign_kernel_ms"] for _ in range(args.repeats)]
    return {"median_ms": round(float(np.median(ms)), 3), "min_ms": round(min(ms), 3), "max_ms": round(max(ms), 3)}


def poisson(R):
    return sal.assign_signatures(X, S, n_resamples=R, resample_seed=1)


def nb(R):
    return sal.nb_assign_signatures(X, S, args.dispersion, n_resamples=R, resample_seed=1)


out = {"data": list(X.shape), "n_signatures": K, "dispersion": args.dispersion, "repeats": args.repeats}
for R in (0, args.resamples):
    a, b = poisson(R), nb(R)
    out[f"R{R}"] = {"assign_signatures": measure(poisson, R), "nb_assign_signatures": measure(nb, R),
                    "problems": int(X.shape[0] * (R + 1)), "iterations": {"assign_signatures": int(a.n_iterations.sum()), "nb_assign_signatures": int(b.n_iterations.sum())},
                    "active": {"assign_signatures": int(a.active.sum()), "nb_assign_signatures": int(b.active.sum())}}
print(json.dumps(out))
