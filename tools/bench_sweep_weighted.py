"""Time a weighted KLNMFSweep (penalty axis) against the same fits one after another, and the weighted batched step
against the unweighted one at 192 x 96.  Prints one JSON line; ``--out`` also writes it to a file.

    python tools/bench_sweep_weighted.py --out profiles/sweep_weighted/bench_sweep_weighted.json
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import salamander_amd as sal  # noqa: E402
from conftest import GOLDEN, read_counts  # noqa: E402
from salamander_amd.batch import BatchEngine  # noqa: E402


def step_time(X, K, members, weighted, steps, repeats):
    N, V = X.shape
    rng = np.random.default_rng(0)
    b = BatchEngine(N, V, [K] * members)
    try:
        b.upload_X(X, clip=True)
        for m in range(members):
            W = rng.uniform(0.1, 1.0, (K, V))
            b.upload_member(m, W / W.sum(axis=1, keepdims=True), rng.uniform(1.0, 100.0, (N, K)))
            if weighted:
                b.set_weights(m, rng.uniform(0.5, 2.0, N), np.full(N, 0.5))
        ids, given = list(range(members)), [0] * members
        b.kl_step(steps, ids, given)
        b.samplewise_kl()  # (waits for the stream)
        times = []
        for _ in range(repeats):
            t0 = time.perf_counter()
            b.kl_step(steps, ids, given)
            b.samplewise_kl()
            times.append((time.perf_counter() - t0) / steps * 1e6)
        return float(np.median(times))
    finally:
        b.close()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--ks", type=int, default=16)
    ap.add_argument("--seeds", type=int, default=2)
    ap.add_argument("--penalties", type=float, nargs="+", default=[0.0, 0.5, 1.0, 2.0])
    ap.add_argument("--skip-sequential", action="store_true")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    X = read_counts(os.path.join(GOLDEN, "pcawg_breast_sbs.csv")).T
    adata = sal.AnnData(X)
    settings = dict(init_method="random")
    Ks, seeds = list(range(1, a.ks + 1)), list(range(a.seeds))
    sal.models.KLNMFSweep([2], seeds=[0], lhalf_weights=[0.5], min_iterations=10, max_iterations=20, **settings).fit(adata)  # warm-up
    s = sal.models.KLNMFSweep(Ks, seeds=seeds, lhalf_weights=a.penalties, **settings)
    t0 = time.perf_counter()
    s.fit(adata)
    sweep_s = time.perf_counter() - t0
    seq_s = None
    if not a.skip_sequential:
        t0 = time.perf_counter()
        for K in Ks:
            for lam in a.penalties:
                for sd in seeds:
                    m = sal.models.KLNMF(K, objective_in_step=False, **settings)
                    m.fit(sal.AnnData(X.copy()), None, {"seed": sd}, {"weights_lhalf": lam})
                    m._engine.close()
        seq_s = time.perf_counter() - t0
    out = {
        "members": len(s.models_), "sweep_s": sweep_s, "timings": s.timings_, "member_steps": s.member_steps_, "sequential_s": seq_s,
        "speedup": None if seq_s is None else seq_s / sweep_s,
        "step_us_192x96_K5_128_members": {"unweighted": step_time(X, 5, 128, False, 2000, 5), "weighted": step_time(X, 5, 128, True, 2000, 5)},
        "step_us_192x96_K5_1_member": {"unweighted": step_time(X, 5, 1, False, 2000, 5), "weighted": step_time(X, 5, 1, True, 2000, 5)},
    }
    line = json.dumps(out)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as fh:
            fh.write(line + "\n")


if __name__ == "__main__":
    main()
