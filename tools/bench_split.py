"""Development aid: KLNMFSweep with count splits against what a user could do without them, on the PCAWG breast catalogue
(192 x 96): K = 1..16 x F = 8 splits, init_method="random", default convergence settings.  Prints one JSON line and writes it
to profiles/sweep/bench_split.json:
(a) the sweep's wall time, split into split / init / batched loop / held-out scoring, with split_s and heldout_s as shares
    of the batched loop;
(b) the baseline: the same 128 fits with the halves thinned on the host (numpy.random.default_rng(seed).binomial over the
    N x V cells per split), KLNMF.fit(objective_in_step=False) one after another on the train halves and the held-out
    divergences by NumPy, in the same process after the same warm-up;
(c) the split kernel alone by device events, in mutations per second, against the host thinning of the same 128 matrices."""
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
from salamander_amd.utils import EPSILON

df = pd.read_csv(os.path.join(ROOT, "tests", "golden", "pcawg_breast_sbs.csv"), index_col=0)
X = np.ascontiguousarray(df.T.values, dtype=np.float64)
adata = sal.AnnData(X.copy())
KS, F, P, SEED = list(range(1, 17)), 8, 0.5, 2024
EPS = float(EPSILON)
counts = X.astype(np.int64)


def host_splits(n, seed):
    rng = np.random.default_rng(seed)
    train = np.stack([rng.binomial(counts, P) for _ in range(n)]).astype(np.float64)
    return train, X[None] - train


def host_heldout(test, W, H):
    x = np.maximum(test, EPS)
    wh = np.maximum((1.0 - P) / P * H, EPS) @ W
    return (x * np.log(x / wh) - x + wh).sum(axis=1)


def sweep():
    s = sal.models.KLNMFSweep(KS, seeds=[0], init_method="random", n_splits=F, train_fraction=P, split_seed=SEED)
    t0 = time.perf_counter()
    models = s.fit(adata)
    wall = time.perf_counter() - t0
    t = s.timings_
    return {"members": len(models), "all_batched": bool(s.batched_.all()), "sweep_s": round(wall, 4), "split_s": round(t["split_s"], 4),
            "init_s": round(t["init_s"], 4), "batched_s": round(t["batched_s"], 4), "heldout_s": round(t["heldout_s"], 4),
            "split_share_of_batched": round(t["split_s"] / t["batched_s"], 4), "heldout_share_of_batched": round(t["heldout_s"] / t["batched_s"], 4),
            "member_steps": int(sum(m.n_iterations_ for m in models)), "heldout_mean": [round(float(v), 3) for v in s.heldout_mean_],
            "suggested": s.suggest_n_signatures_heldout(), "suggested_one_standard_error": s.suggest_n_signatures_heldout(True)}


def sweep_without_splits():
    """The same number of members on the parent's path: 8 seeds instead of 8 splits."""
    s = sal.models.KLNMFSweep(KS, seeds=list(range(F)), init_method="random")
    t0 = time.perf_counter()
    models = s.fit(adata)
    return {"members": len(models), "sweep_s": round(time.perf_counter() - t0, 4), "init_s": round(s.timings_["init_s"], 4),
            "batched_s": round(s.timings_["batched_s"], 4), "member_steps": int(sum(m.n_iterations_ for m in models))}


def baseline():
    t0 = time.perf_counter()
    train, test = host_splits(F, SEED)
    t_draw = time.perf_counter() - t0
    steps, t_score = 0, 0.0
    for K in KS:
        for f in range(F):
            m = sal.models.KLNMF(K, "random", objective_in_step=False)
            m.fit(sal.AnnData(train[f].copy()), init_kwargs={"seed": 0})
            steps += m.n_iterations_
            m._engine.close()
            ta = time.perf_counter()
            host_heldout(test[f], np.asarray(m.asignatures.X), np.asarray(m.adata.obsm["exposures"]))
            t_score += time.perf_counter() - ta
    return {"sequential_s": round(time.perf_counter() - t0, 4), "host_split_s": round(t_draw, 4), "host_heldout_s": round(t_score, 4),
            "member_steps": int(steps)}


def kernel_alone(n_matrices=128, n_calls=20):
    mutations = int(counts.sum()) * n_matrices
    b = BatchEngine(X.shape[0], X.shape[1], [1])
    try:
        b.upload_X(X, clip=True)
        ms = b.profile_split(n_matrices, P, SEED, n_calls)
    finally:
        b.close()
    host_splits(1, 1)
    t0 = time.perf_counter()
    host_splits(n_matrices, SEED)
    host_s = time.perf_counter() - t0
    return {"matrices": n_matrices, "mutations": mutations, "kernel_ms": round(ms, 4), "kernel_mutations_per_s": round(mutations / (ms * 1e-3), 1),
            "host_s": round(host_s, 4), "host_mutations_per_s": round(mutations / host_s, 1), "factor": round(host_s / (ms * 1e-3), 1)}


# warm-up: every shape and code path of the timed windows
sal.models.KLNMFSweep([1, 5, 16], seeds=[0], init_method="random", min_iterations=20, max_iterations=20, n_splits=2).fit(adata)
for K in (1, 5, 16):
    w = sal.models.KLNMF(K, "random", objective_in_step=False, min_iterations=20, max_iterations=20)
    w.fit(sal.AnnData(X.copy()), init_kwargs={"seed": 0})
    w._engine.close()
out = {"data": list(X.shape), "ns_signatures": [KS[0], KS[-1]], "n_splits": F, "train_fraction": P, "mutations": int(counts.sum())}
out["sweep"] = sweep()
out["sweep_again"] = sweep()
out["sweep_without_splits"] = sweep_without_splits()
out["baseline"] = baseline()
out["speedup_wall"] = round(out["baseline"]["sequential_s"] / out["sweep_again"]["sweep_s"], 2)
out["split_kernel"] = kernel_alone()
line = json.dumps(out)
print(line, flush=True)
dest = os.path.join(ROOT, "profiles", "sweep")
os.makedirs(dest, exist_ok=True)
with open(os.path.join(dest, "bench_split.json"), "w") as fh:
    fh.write(line + "\n")
