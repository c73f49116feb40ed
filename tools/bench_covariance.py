"""Development aid: sal.exposure_covariance against the host path for the same job -- a batched NumPy Gram matrix
(einsum) and np.linalg.inv per sample.  Two workloads: the PCAWG breast catalogue (192 x 96) against the consensus signatures of
a small sweep, and a synthetic cohort of 10 000 samples with K = 64.  The exposures come from sal.refit_exposures and are passed
in, so only the covariance is timed.  The kernel time is by device events, the median of 7 calls after a warm-up (min and max
alongside); the host path is timed once per workload.  Prints one JSON line and writes it to --out (default
profiles/covariance/bench_covariance.json)."""
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

EPSILON = float(np.finfo(np.float32).eps)
ap = argparse.ArgumentParser()
ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "covariance", "bench_covariance.json"))
ap.add_argument("--skip-large", action="store_true")
ap.add_argument("--calls", type=int, default=7)
args = ap.parse_args()


def host_path(X, W, H, information):
    """Standard errors and inflation of every sample, all signatures active: one einsum for the Gram matrices, one inverse each"""
    t0 = time.perf_counter()
    x = np.maximum(X, EPSILON)
    p = np.maximum(H @ W, EPSILON)
    d = x / (p * p) if information == "observed" else 1.0 / p
    J = np.einsum("kv,nv,lv->nkl", W, d, W, optimize=True)
    D = np.einsum("nkk->nk", J)
    C = J / np.sqrt(D[:, :, None] * D[:, None, :])
    t_gram = time.perf_counter() - t0
    infl = np.empty_like(D)
    for n in range(X.shape[0]):
        infl[n] = np.diag(np.linalg.inv(C[n]))
    total = time.perf_counter() - t0
    return np.sqrt(infl / D), {"gram_s": round(t_gram, 4), "total_s": round(total, 4)}


def device_path(X, W, H, information, return_correlation):
    sal.exposure_covariance(X[:32], W, H[:32], information=information)  # warm-up
    ms, wall = [], []
    for _ in range(args.calls):
        res = sal.exposure_covariance(X, W, H, information=information, return_correlation=return_correlation)
        ms.append(res.timings["information_kernel_ms"])
        wall.append(res.timings["total_s"])
    return res, {"kernel_ms_median": round(float(np.median(ms)), 4), "kernel_ms_min": round(min(ms), 4), "kernel_ms_max": round(max(ms), 4),
                 "wall_s_median": round(float(np.median(wall)), 4), "n_chunks": res.timings["n_chunks"], "calls": args.calls}


def workload(name, X, S):
    W = S / S.sum(axis=1, keepdims=True)
    H = sal.refit_exposures(X, S).exposures
    out = {"data": list(X.shape), "K": int(S.shape[0])}
    for information in ("observed", "expected"):
        res, dev = device_path(X, S, H, information, False)
        _, dev_corr = device_path(X, S, H, information, True)
        se, host = host_path(X, W, H, information)
        ok = ~res.singular
        agree = float(np.nanmax(np.abs(res.standard_errors[ok] / se[ok] - 1.0))) if ok.any() else None
        out[information] = {"device": dev, "device_with_correlation": dev_corr, "host": host, "singular": int(res.singular.sum()),
                            "largest_inflation": float(np.nanmax(res.inflation)) if ok.any() else None, "standard_errors_max_rel_diff": agree}
        print(f"# {name} {information}: {json.dumps(out[information])}", file=sys.stderr, flush=True)
    return out


df = pd.read_csv(os.path.join(ROOT, "tests", "golden", "pcawg_breast_sbs.csv"), index_col=0)
Xp = np.ascontiguousarray(df.T.values, dtype=np.float64)
adata = sal.AnnData(Xp.copy())
adata.var_names = list(df.index)
sweep = sal.models.KLNMFSweep(ns_signatures=[10], seeds=[0, 1, 2], stability=True, min_iterations=200, max_iterations=400)
sweep.fit(adata)
result = {"pcawg": workload("pcawg", Xp, np.asarray(sweep.consensus_signatures_[0], dtype=np.float64))}
if not args.skip_large:
    rng = np.random.default_rng(0)
    Ss = rng.dirichlet(np.full(96, 0.2), size=64) + 1e-5
    Ss /= Ss.sum(axis=1, keepdims=True)
    E = rng.dirichlet(np.full(64, 0.1), size=10000) * rng.uniform(500, 20000, size=(10000, 1))
    Xs = rng.poisson(E @ Ss).astype(np.float64)
    result["synthetic"] = workload("synthetic", Xs, Ss)
line = json.dumps(result)
print(line, flush=True)
os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
with open(args.out, "w") as fh:
    fh.write(line + "\n")
