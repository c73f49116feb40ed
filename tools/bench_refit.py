"""Development aid: sal.refit_exposures against what the package offered before it for the same job -- resamples drawn on
the host and R + 1 calls of KLNMF(K, objective_in_step=False).fit(..., given_parameters={"asignatures": S}).  Two
workloads: the PCAWG breast catalogue (192 x 96) with K = 8 and R = 100 (baseline timed on 21 fits), and a synthetic cohort of 10 000 samples with
K = 64 (R = 8; its baseline is timed on `--baseline-fits` fits and scaled to R + 1, marked "extrapolated").  Each at a
fixed step count (min = max = 200 iterations) and at the defaults.  Prints one JSON line and writes it to --out: wall time
of both, the refit kernel's time by device events, its rate counted as 4 V K flops per problem-step, and that rate against
the fp64 matrix peak of an MI355X (78.6 TFLOP/s).  One rocprofv3 --kernel-trace --stats run of this script shows the two
kernels' shares."""
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

PEAK_FP64_MFMA = 78.6e12
ap = argparse.ArgumentParser()
ap.add_argument("--out", default=None)
ap.add_argument("--baseline-fits", type=int, default=3)
ap.add_argument("--skip-large", action="store_true")
args = ap.parse_args()


def host_resamples(X, n, seed):
    rng = np.random.default_rng(seed)
    totals = X.sum(axis=1).astype(np.int64)
    P = X / X.sum(axis=1, keepdims=True)
    return np.stack([np.stack([rng.multinomial(totals[i], P[i]) for i in range(len(X))]) for _ in range(n)]).astype(np.float64)


def baseline(X, S, R, n_fits, **kw):
    """R + 1 sequential fits with all signatures given (n_fits of them timed; the rest scaled)."""
    sigs = sal.AnnData(S.copy())
    t0 = time.perf_counter()
    mats = [X] + list(host_resamples(X, min(R, n_fits - 1), 1)) if n_fits > 1 else [X]
    t_draw = time.perf_counter() - t0
    steps = 0
    t0 = time.perf_counter()
    for m_ in mats:
        m = sal.models.KLNMF(S.shape[0], objective_in_step=False, **kw)
        m.fit(sal.AnnData(m_.copy()), given_parameters={"asignatures": sigs})
        steps += m.n_iterations_
        m._engine.close()
    per_fit = (time.perf_counter() - t0) / len(mats)
    per_draw = t_draw / max(1, len(mats) - 1)
    return {"fits_timed": len(mats), "per_fit_s": round(per_fit, 4), "steps_per_fit": steps / len(mats), "host_draw_per_resample_s": round(per_draw, 4),
            "total_s": round(per_fit * (R + 1) + per_draw * R, 4), "extrapolated": len(mats) < R + 1}


def refit(X, S, R, **kw):
    sal.refit_exposures(X[:32], S, n_resamples=2, min_iterations=5, max_iterations=5)  # warm-up
    res = sal.refit_exposures(X, S, n_resamples=R, **kw)
    V, K = X.shape[1], S.shape[0]
    steps = int(res.n_iterations.sum()) + int(res.n_iterations_resampled.sum())
    flops = 4.0 * V * K * steps
    ms = res.timings["refit_kernel_ms"]
    return {"wall_s": round(res.timings["total_s"], 4), "resample_s": round(res.timings["resample_s"], 5), "refit_kernel_ms": round(ms, 3),
            "reduce_s": round(res.timings["reduce_s"], 5), "n_chunks": res.timings["n_chunks"], "problem_steps": steps,
            "median_iterations": float(np.median(res.n_iterations_resampled)), "not_converged": int((res.n_iterations_resampled >= kw.get("max_iterations", 10000)).sum()),
            "tflops": round(flops / (ms * 1e-3) / 1e12, 3), "of_fp64_mfma_peak": round(flops / (ms * 1e-3) / PEAK_FP64_MFMA, 4)}


def workload(name, X, S, R, n_fits):
    out = {"data": list(X.shape), "K": S.shape[0], "R": R}
    for label, kw in (("fixed_200", dict(min_iterations=200, max_iterations=200)), ("defaults", {})):
        r = refit(X, S, R, **kw)
        b = baseline(X, S, R, n_fits, **kw)
        out[label] = {"refit": r, "baseline": b, "speedup_wall": round(b["total_s"] / r["wall_s"], 1)}
        print(f"# {name} {label}: {json.dumps(out[label])}", file=sys.stderr, flush=True)
    return out


df = pd.read_csv(os.path.join(ROOT, "tests", "golden", "pcawg_breast_sbs.csv"), index_col=0)
Xp = np.ascontiguousarray(df.T.values, dtype=np.float64)
rng = np.random.default_rng(0)
Sp = rng.dirichlet(np.full(96, 0.2), size=8) + 1e-5
result = {"pcawg": workload("pcawg", Xp, Sp / Sp.sum(axis=1, keepdims=True), 100, 21)}
if not args.skip_large:
    Ss = rng.dirichlet(np.full(96, 0.2), size=64) + 1e-5
    Ss /= Ss.sum(axis=1, keepdims=True)
    E = rng.dirichlet(np.full(64, 0.1), size=10000) * rng.uniform(500, 20000, size=(10000, 1))
    Xs = rng.poisson(E @ Ss).astype(np.float64)
    result["synthetic"] = workload("synthetic", Xs, Ss, 8, args.baseline_fits)
line = json.dumps(result)
print(line, flush=True)
if args.out:
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as fh:
        fh.write(line + "\n")
