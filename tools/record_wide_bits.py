"""Record what engines with feature blocks (> 96 features), signature chunks (> 64 signatures) or both compute, bit for bit.

Every case drives ``salamander_amd.Engine`` through one fixed script (``sync()`` between the steps) and records the SHA-256 of
the raw bytes of every array it downloads and every scalar it gets back as a hex float.  The passes use no atomics and
fixed-order sums, so a build computes the same record on every run, and a change of the host code that
issues the same launches computes the same record as the build before it: ``tests/test_gpu_wide_bits.py`` compares with
``tests/golden/wide_bits.json``, written by

    python tools/record_wide_bits.py [path of the record]

on a build known to be right (run it twice: the two records must be identical).
"""
import hashlib
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np

from salamander_amd import Engine, _lib
from salamander_amd.synthetic import synthetic_problem

N = 333  # 21 tiles of 16 samples, the last one partial
GOLDEN = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tests", "golden", "wide_bits.json")

# (kind, V, K, n_given | dim): the smallest shapes that reach each branch of the wide host logic
CASES = [
    ("kl", 96, 5, 0),  # control: one block, one chunk
    ("kl", 97, 18, 0),  # two blocks (first and last), a ragged last block of one column, remainder columns
    ("kl", 200, 5, 2),  # three blocks (first, middle, last)
    ("kl", 200, 5, 5),  # ... every signature given: W untouched
    ("kl", 96, 65, 0),  # chunks of 33 + 32
    ("kl", 90, 100, 3),  # chunks of 50 + 50 with remainder columns
    ("kl", 96, 130, 50),  # three chunks: the first wholly given (skipped where only W is updated), the second partly
    ("kl", 96, 120, 0),  # chunks of 60 + 60 on the deepest contraction
    ("kl", 200, 100, 0),  # blocks and chunks
    ("kl", 200, 100, 3),
    ("kl", 97, 130, 50),
    ("weighted", 200, 5, 2),
    ("weighted", 96, 65, 0),
    ("weighted", 200, 100, 3),
    ("corr", 200, 7, 3),  # CorrNMF on feature blocks
]


def case_name(case):
    kind, V, K, last = case
    return f"{kind}-V{V}-K{K}-{'dim' if kind == 'corr' else 'given'}{last}"


def _digest(a):
    return hashlib.sha256(np.ascontiguousarray(a, dtype=np.float64).tobytes()).hexdigest()


def _run_kl(e, rec, n_given):
    rec("objective", e.objective())
    e.kl_step(3, n_given)
    e.sync()
    e.update_H()
    e.sync()
    e.update_W(n_given)
    e.sync()
    rec("W after the steps", e.download_W())
    rec("H after the steps", e.download_H())
    e.kl_step_keep(2, n_given)
    e.sync()
    rec("W kept block", e.download_W())
    rec("H kept block", e.download_H())
    e.kl_rollback()
    e.sync()
    rec("W rolled back", e.download_W())
    rec("H rolled back", e.download_H())
    e.kl_step_objective(1, 1, n_given)
    rec("objective_read", e.objective_read(1, 1))
    e.sync()
    rec("samplewise_kl", e.samplewise_kl())
    rec("reconstruct", e.reconstruct())
    try:  # (a build that refuses the MvNMF steps of this engine stops here, and says so in the record)
        rec("mv_step gamma", e.mv_step(2, n_given, 1.0, 1.0, 1.0))
        e.sync()
        rec("mv_objective", e.mv_objective(1.0, 1.0))
    except RuntimeError as err:
        rec("mvnmf refused", str(err))
    rec("W", e.download_W())
    rec("H", e.download_H())


def _run_corr(e, rec, rng, X, K, dim):
    beta = rng.normal(0.0, 0.3, size=K)
    alpha = np.log(X.sum(axis=1) / K) + rng.normal(0.0, 0.1, size=N)
    L, U = rng.normal(0.0, 0.5, size=(K, dim)), rng.normal(0.0, 0.5, size=(N, dim))
    e.corr_configure(dim)
    for which, a in ((_lib.CORR_SIGNATURE_SCALINGS, beta), (_lib.CORR_SAMPLE_SCALINGS, alpha), (_lib.CORR_SIGNATURE_EMBEDDINGS, L), (_lib.CORR_SAMPLE_EMBEDDINGS, U)):
        e.corr_upload(which, a)
    e.corr_compute_exposures()
    e.sync()
    e.corr_compute_aux()
    e.sync()
    rec("aux", e.corr_download(_lib.CORR_AUX))
    e.corr_update_signatures(0)
    e.sync()
    rec("W after update_signatures(0)", e.download_W())
    e.corr_update_signatures(2)
    e.sync()
    rec("W after update_signatures(2)", e.download_W())
    rec("H", e.download_H())


def run_case(case):
    """The record of one case: a list of [label, SHA-256 of an array's bytes | hex float | text]."""
    kind, V, K, last = case
    X, W0, H0 = synthetic_problem(V, N, K, seed=1000 + V + K)
    rng = np.random.default_rng(V + K)
    out = []

    def rec(label, value):
        if isinstance(value, str):
            out.append([label, value])
        elif np.ndim(value) == 0:
            out.append([label, float(value).hex()])
        else:
            out.append([label, _digest(value)])

    e = Engine(N, V, K)
    e.upload_X(X), e.upload_W(W0), e.upload_H(H0)
    if kind == "weighted":
        e.set_weights(rng.uniform(0.5, 2.0, N), rng.uniform(0.0, 0.4, N))
    if kind == "corr":
        _run_corr(e, rec, rng, X, K, last)
    else:
        _run_kl(e, rec, last)
    e.close()
    return out


if __name__ == "__main__":
    path = sys.argv[1] if len(sys.argv) > 1 else GOLDEN
    record = {case_name(c): run_case(c) for c in CASES}
    with open(path, "w") as fh:
        json.dump(record, fh, indent=1)
        fh.write("\n")
    print(f"{len(record)} cases, {sum(len(v) for v in record.values())} entries -> {path}")
