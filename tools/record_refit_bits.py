"""Record what the refit family computes, bit for bit: ``refit_exposures``, ``assign_signatures`` (plain, and with candidates,
required signatures and the re-addition pass), ``goodness_of_fit``, ``signature_presence_test``, ``signature_power``,
``profile_likelihood`` and ``exposure_intervals``.

The seven entry points share one tile-solve skeleton (``csrc/salnmf_refit.h``) and one host kit (``csrc/salnmf_refit.hip``).
Their kernels use no atomics in their arithmetic and fixed-order sums, and a problem's result depends on its row and the
signatures alone, so a build computes the same record on every run, and a change that moves their code without changing an
operation computes the same record as the build before it: ``tests/test_gpu_refit_family_bits.py`` compares with
``tests/golden/refit_family_bits.npz``, written by

    python tools/record_refit_bits.py [path of the record]

on a build known to be right (run it twice: the two records must be identical).

Shapes: 37 samples (three tiles of 16, the last ragged, fewer tiles than a workgroup has waves); 96 features, and 83 at 17 and
96 signatures; 5, 17, 40, 50, 70 and 96 signatures, one per instantiation of the kernels (KT = 1 .. 6).  The inputs come from
the integer hash below (no library's random stream is part of the record).  The record holds every array an entry point
returns and the counts its ``timings`` carry (never the milliseconds): in the cases ``FULL_CASES`` every array as it is; in the
others an array of at most ``FULL`` entries as it is, a larger one as the SHA-256 of its dtype, shape and bytes -- equal digests
are equal bits, NaN payloads included -- which keeps the record within the size of a committed file.
"""
import dataclasses
import hashlib
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np

GOLDEN = os.path.join(ROOT, "tests", "golden", "refit_family_bits.npz")

N = 37
CASES = [(96, 5), (96, 17), (83, 17), (96, 40), (96, 50), (96, 70), (96, 96), (83, 96)]  # (V, K)
FULL = 256  # entries of the largest array the record holds as it is, in a case that is not one of FULL_CASES
FULL_CASES = [(96, 5), (96, 17)]  # held in full, whatever the size: a failing array there shows where and by how much it differs
ITER = dict(min_iterations=10, max_iterations=40, conv_test_freq=10)
# per signature count, a tolerance at which some columns of the dense refit stop at a test (20 or 30 iterations) and others
# run to 40: more signatures converge more slowly (chosen on the host replica tests/_refit_ref.py, free-running)
TOL = {5: 0.005, 17: 0.02, 40: 0.03, 50: 0.05, 70: 0.05, 96: 0.1}
B = 5  # resamples, null draws
SHARES, ALT = (0.0, 0.1), 3
ALPHA = 0.4  # max_exceed = 1 of 5
VALUES = (0.0, 0.5, 3.0, 20.0, 150.0)
LONG_RUN_CASE = (96, 17)  # its profile takes PROFILE_RUN + 1 = 9 values per pair, given pair by pair: a pair spans two runs
SEARCH = dict(max_kl_increase=1.92, n_bisections=4, max_expansions=6)
ENTRIES = ("refit", "assign", "assign_masks", "gof", "presence", "power", "profile", "intervals")


def case_name(case):
    return f"V{case[0]}-K{case[1]}"


def case_seed(case):
    return 7000 + 100 * case[0] + case[1]


def uniform(seed, *shape):
    """``shape`` numbers in [0, 1): the top 53 bits of splitmix64 of ``seed * 2^32 + index``, in uint64 arithmetic."""
    n = int(np.prod(shape))
    with np.errstate(over="ignore"):
        z = (np.arange(n, dtype=np.uint64) + np.uint64(seed << 32)) * np.uint64(0x9E3779B97F4A7C15) + np.uint64(0x9E3779B97F4A7C15)
        z = (z ^ (z >> np.uint64(30))) * np.uint64(0xBF58476D1CE4E5B9)
        z = (z ^ (z >> np.uint64(27))) * np.uint64(0x94D049BB133111EB)
        z = z ^ (z >> np.uint64(31))
    return ((z >> np.uint64(11)).astype(np.float64) / float(1 << 53)).reshape(shape)


def inputs(case):
    """(counts (N, V) of integer values with zeros, signatures (K, V), test (2,), candidates (N, K) bool, required (N, K) bool)."""
    V, K = case
    seed = case_seed(case)
    W = uniform(seed, K, V) ** 6 + 1e-3
    W = W / W.sum(axis=1, keepdims=True)
    E = np.where(uniform(seed + 1, N, K) < 0.35, uniform(seed + 2, N, K), 0.0)
    E[np.arange(N), np.arange(N) % K] += 0.5  # no empty sample
    E = E / E.sum(axis=1, keepdims=True) * (150.0 + 6000.0 * uniform(seed + 3, N, 1) ** 2)
    X = np.floor((E @ W) * (0.4 + 1.2 * uniform(seed + 4, N, V)))
    X[uniform(seed + 5, N, V) < 0.03] = 0.0
    X[:, 0] += X.sum(axis=1) == 0  # (no empty row)
    test = np.array([1, K - 2], dtype=np.int32)
    C = uniform(seed + 6, N, K) < 0.6
    C[:, test[0]] = True
    C[2:, test[1]] = uniform(seed + 7, N - 2) < 0.8
    C[0] = False
    C[0, test[0]] = True  # a single candidate: both of its pairs are untested
    C[1, test[1]] = False  # a tested signature outside the set
    C[1, 0] = True
    Rq = C & (uniform(seed + 8, N, K) < 0.2)
    return X, W, test, C, Rq


def tested_pairs(test, C):
    return int((C[:, test] & (C.sum(axis=1, keepdims=True) > 1)).sum())


def flatten(prefix, result, out):
    """Every array of a result (and of the results inside it) and the counts of its timings, by name."""
    for f in dataclasses.fields(result):
        value = getattr(result, f.name)
        if dataclasses.is_dataclass(value):
            flatten(f"{prefix}/{f.name}", value, out)
        elif isinstance(value, np.ndarray):
            out[f"{prefix}/{f.name}"] = value
        elif f.name == "timings":
            for key in ("n_chunks", "n_alt_chunks", "n_problems"):
                if key in value:
                    out[f"{prefix}/{key}"] = np.array([value[key]], dtype=np.int64)


def encode(arrays, full=False):
    out = {}
    for name, a in arrays.items():
        a = np.ascontiguousarray(a)
        if full or a.size <= FULL:
            out[name] = a
        else:
            head = f"{a.dtype.str}{a.shape}".encode()
            out[name + "#sha256"] = np.frombuffer(hashlib.sha256(head + a.tobytes()).digest(), dtype=np.uint8)
    return out


def run_case(case):
    """name -> array (or digest) of everything the calls of one case return (the seven entry points, the assignment twice)."""
    import salamander_amd as sal
    from salamander_amd.assign import assign_signatures
    from salamander_amd.gof import goodness_of_fit
    from salamander_amd.intervals import exposure_intervals, profile_likelihood
    from salamander_amd.power import signature_power
    from salamander_amd.presence import signature_presence_test
    from salamander_amd.refit import refit_exposures

    del sal
    V, K = case
    X, W, test, C, Rq = inputs(case)
    it = dict(ITER, tol=TOL[K])
    rows = 2 * 8 * N * V + 8  # two resamples (draws) of the sample list per chunk: three chunks for five
    pair_rows = 2 * 8 * tested_pairs(test, C) * V + 8  # ... of the pair list: three chunks for five draws and for 2 x 3 alternative draws
    if case == LONG_RUN_CASE:
        values = 40.0 * uniform(case_seed(case) + 9, N, 2, 9) ** 2
        values[:, :, 0] = 0.0
    else:
        values = np.array(VALUES)
    results = {
        "refit": refit_exposures(X, W, n_resamples=B, resample_seed=11, keep_resamples=True, chunk_bytes=rows, **it),
        "assign": assign_signatures(X, W, n_resamples=B, resample_seed=12, keep_resamples=True, chunk_bytes=rows, **it),
        "assign_masks": assign_signatures(X, W, n_resamples=B, resample_seed=13, keep_resamples=True, chunk_bytes=rows, candidates=C,
                                          required=Rq, readd=True, **it),
        "gof": goodness_of_fit(X, W, n_draws=B, seed=14, keep_draws=True, chunk_bytes=rows, **it),
        "presence": signature_presence_test(X, W, test, n_draws=B, seed=15, candidates=C, keep_draws=True, chunk_bytes=pair_rows, **it),
        "power": signature_power(X, W, test, shares=SHARES, n_draws=B, n_alt_draws=ALT, alpha=ALPHA, candidates=C, seed=16, keep_draws=True,
                                 chunk_bytes=pair_rows, **it),
        "profile": profile_likelihood(X, W, test, values, candidates=C, keep_exposures=True, **it),
        "intervals": exposure_intervals(X, W, test, candidates=C, keep_trace=True, **SEARCH, **it),
    }
    assert tuple(results) == ENTRIES
    for name in ("refit", "assign", "assign_masks", "gof", "presence"):
        assert results[name].timings["n_chunks"] == 3, (name, results[name].timings)
    assert results["power"].presence.timings["n_chunks"] == 3 and results["power"].timings["n_alt_chunks"] == 3
    for name in ("refit", "gof"):  # the dense refit: some columns stop at a test before the last, others run to max_iterations
        nit = results[name].n_iterations
        assert (nit < ITER["max_iterations"]).any() and (nit == ITER["max_iterations"]).any(), (name, np.bincount(nit))
    tested = results["presence"].tested
    assert not tested[0].any() and tested[1, 0] and not tested[1, 1]  # untested pairs: a set of one, a signature outside the set
    arrays = {}
    for name, result in results.items():
        flatten(name, result, arrays)
    return encode(arrays, full=case in FULL_CASES)


def record():
    out = {"seeds": np.array([case_seed(c) for c in CASES], dtype=np.int64)}
    for case in CASES:
        for name, a in run_case(case).items():
            out[f"{case_name(case)}/{name}"] = a
    return out


if __name__ == "__main__":
    path = sys.argv[1] if len(sys.argv) > 1 else GOLDEN
    rec = record()
    np.savez_compressed(path, **rec)
    print(f"{len(CASES)} cases, {len(rec)} entries, {os.path.getsize(path)} bytes -> {path}")
    assert os.path.getsize(path) < (1 << 20), "the record must stay below 1 MiB"
