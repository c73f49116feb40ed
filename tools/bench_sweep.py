"""Development aid: KLNMFSweep against the tutorial's loop of single fits (tutorial.ipynb section 1.6) on the PCAWG breast
catalogue (192 x 96): K = 1..16 x 8 seeds, init_method="random".  Prints one JSON line: wall time of the batched sweep
(initialisation split out), wall time of the same 128 fits one after another through KLNMF.fit (objective_in_step=False,
the sweep's contract), member-steps and member-steps/s of both -- at the default convergence settings and with
min_iterations = max_iterations = 1000 (step throughput alone)."""
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np
import pandas as pd

import salamander_amd as sal

df = pd.read_csv(os.path.join(ROOT, "tests", "golden", "pcawg_breast_sbs.csv"), index_col=0)
adata = sal.AnnData(df.T.values.astype(float))
KS, SEEDS = list(range(1, 17)), list(range(8))


def run(settings):
    s = sal.models.KLNMFSweep(KS, seeds=SEEDS, init_method="random", **settings)
    t0 = time.perf_counter()
    models = s.fit(adata)
    sweep_s = time.perf_counter() - t0
    steps = int(sum(m.n_iterations_ for m in models))
    t0 = time.perf_counter()
    seq_steps = 0
    for K in KS:
        for seed in SEEDS:
            m = sal.models.KLNMF(K, "random", objective_in_step=False, **settings)
            m.fit(adata.copy(), init_kwargs={"seed": seed})
            seq_steps += m.n_iterations_
            m._engine.close()
    seq_s = time.perf_counter() - t0
    return {
        "members": len(models), "all_batched": bool(s.batched_.all()),
        "sweep_s": round(sweep_s, 4), "sweep_init_s": round(s.timings_["init_s"], 4), "sweep_batched_s": round(s.timings_["batched_s"], 4),
        "sequential_s": round(seq_s, 4), "member_steps": steps, "sequential_member_steps": int(seq_steps),
        "sweep_member_steps_per_s": round(steps / sweep_s, 1), "sweep_loop_member_steps_per_s": round(steps / s.timings_["batched_s"], 1),
        "sequential_member_steps_per_s": round(seq_steps / seq_s, 1), "speedup_wall": round(seq_s / sweep_s, 2),
    }


sal.models.KLNMFSweep([1, 5], seeds=[0], init_method="random", min_iterations=20, max_iterations=20).fit(adata)  # (warm-up)
out = {"data": list(adata.X.shape), "ns_signatures": [KS[0], KS[-1]], "seeds": len(SEEDS)}
out["converged"] = run({})
out["fixed_1000"] = run({"min_iterations": 1000, "max_iterations": 1000})
print(json.dumps(out), flush=True)
