"""Per-problem host reference of the CorrNMF embedding solves, and the checks that compare a device result with it.

``tests/native/ncg_ref_host.cpp`` runs ``csrc/salnmf_ncg_machine.h`` -- the Newton-CG of every device form -- with an
evaluator in long double, once unperturbed (the reference) and ``N_PERT`` times with every evaluation perturbed by
``DELTA`` times its own magnitude (antithetic pairs).  ``DELTA`` sits about 100x above the device's evaluation error at
up to 128 terms.  A problem whose runs all end with the same status and within ``SPREAD`` of each other is *stable*:
no termination or line-search test of its solve lies within rounding of its threshold, and the device must reproduce
the reference to ``TOL_STABLE`` with the same status.  On an *unstable* problem a rounding difference may legitimately
take another decision; the device must then reproduce ONE of the runs to ``TOL_UNSTABLE`` or to the ensemble's own
scatter.  Stability also requires the same number of solver rounds in every run: a flipped CG or line-search test
changes it even where the iterate moves little.

Errors are relative to ``max(|x|_inf, 1e-3)`` of the reference.  The calibration record (measured maxima per case) is
in the commit that introduced these tests; the GPU tests print it again on every run.
"""

from __future__ import annotations

import hashlib
import os
import shutil
import subprocess
import tempfile
from dataclasses import dataclass

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "native", "ncg_ref_host.cpp")
MACHINE = os.path.join(ROOT, "salamander_amd", "csrc", "salnmf_ncg_machine.h")

EPSILON = float(np.finfo(np.float32).eps)
N_PERT = 8
DELTA = 1e-12
SPREAD = 1e-7  # ensemble spread below which a same-path problem counts as stable: drift ~ DELTA cond reaches 2e-9, a flipped decision jumps 1e-5 and more
TOL_STABLE = 1e-11
TOL_UNSTABLE = 1e-9
MAX_UNSTABLE = 0.05
THREADS = 16

_exe = None


def compiler() -> str:
    """g++, else ROCm's clang++: the host reference never goes missing where the library builds."""
    for c in (shutil.which("g++"), os.path.join(os.environ.get("ROCM_PATH", "/opt/rocm"), "llvm", "bin", "clang++"), "/opt/rocm/llvm/bin/clang++"):
        if c and os.path.exists(c):
            return c
    raise RuntimeError("no host C++ compiler (g++ or ROCm's clang++) for tests/native/ncg_ref_host.cpp")


def executable() -> str:
    global _exe
    if _exe is None:
        h = hashlib.sha256()
        for p in (SRC, MACHINE):
            h.update(open(p, "rb").read())
        d = os.path.join(tempfile.gettempdir(), f"salnmf_ncg_ref_{os.getuid()}")
        os.makedirs(d, exist_ok=True)
        exe = os.path.join(d, f"ncg_ref_{h.hexdigest()[:16]}")
        if not os.path.exists(exe):
            tmp = f"{exe}.{os.getpid()}"
            subprocess.run([compiler(), "-O2", "-std=c++17", "-pthread", "-o", tmp, SRC], check=True)
            os.replace(tmp, exe)
        _exe = exe
    return _exe


def push_eps(x):
    """The push of entries within EPSILON of zero to +-EPSILON (``_utils_corrnmf.py:408-409``), as the device applies it."""
    x = np.array(x, dtype=np.float64, copy=True)
    x[(0 < x) & (x < EPSILON)] = EPSILON
    x[(-EPSILON < x) & (x < 0)] = -EPSILON
    return x


class Problems:
    """A batch of general embedding problems: term matrices by index, per problem offsets / aux / start point."""

    def __init__(self):
        self.mats, self.probs = [], []

    def matrix(self, L) -> int:
        self.mats.append(np.ascontiguousarray(L, dtype=np.float64))
        return len(self.mats) - 1

    def add(self, mat: int, off, aux, x0, variance: float, maxiter: int):
        T, dim = self.mats[mat].shape
        off, aux, x0 = (np.ascontiguousarray(v, dtype=np.float64).ravel() for v in (off, aux, x0))
        assert off.shape == (T,) and aux.shape == (T,) and x0.shape == (dim,)
        self.probs.append((mat, int(maxiter), float(variance), off, aux, x0))

    def dim(self, p: int) -> int:
        return self.mats[self.probs[p][0]].shape[1]

    def __len__(self):
        return len(self.probs)


def sample_problems(L, off, aux, U0, variance, maxiter, probs: Problems | None = None) -> Problems:
    """One problem per sample: terms = the T signatures (of all modalities), ``off (N, T)``, ``aux (N, T)``, ``U0 (N, dim)``."""
    probs = probs or Problems()
    m = probs.matrix(L)
    for n in range(U0.shape[0]):
        probs.add(m, off[n], aux[n], U0[n], variance, maxiter)
    return probs


def signature_problems(U, alpha, beta, aux, L0, variance, maxiter, probs: Problems | None = None) -> Problems:
    """One problem per signature k: terms = the N samples, offsets alpha_n + beta_k, ``aux (N, K)``, start point L0[k]."""
    probs = probs or Problems()
    m = probs.matrix(U)
    for k in range(L0.shape[0]):
        probs.add(m, alpha + beta[k], aux[:, k], L0[k], variance, maxiter)
    return probs


@dataclass
class Reference:
    x: list  # per problem (runs, dim): run 0 unperturbed
    status: np.ndarray  # (P, runs)
    rounds: np.ndarray
    points: np.ndarray  # point evaluations per run
    stable: np.ndarray  # (P,)
    spread: np.ndarray  # (P,)

    @property
    def ref(self):
        return [xr[0] for xr in self.x]


def scale_of(x):
    return max(float(np.abs(x).max()), 1e-3)


def solve(probs: Problems, n_pert: int = N_PERT, delta: float = DELTA, threads: int = THREADS) -> Reference:
    with tempfile.TemporaryDirectory() as d:
        fin, fout = os.path.join(d, "in.bin"), os.path.join(d, "out.bin")
        with open(fin, "wb") as f:
            f.write(np.array([len(probs.mats), len(probs.probs), n_pert], dtype="<i4").tobytes())
            f.write(np.array([delta], dtype="<f8").tobytes())
            for L in probs.mats:
                f.write(np.array(L.shape, dtype="<i4").tobytes())
                f.write(L.astype("<f8").tobytes())
            for mat, maxiter, var, off, aux, x0 in probs.probs:
                f.write(np.array([mat, maxiter], dtype="<i4").tobytes())
                f.write(np.concatenate([[var], off, aux, x0]).astype("<f8").tobytes())
        subprocess.run([executable(), fin, fout, str(threads)], check=True)
        raw = open(fout, "rb").read()
    runs = n_pert + 1
    P = len(probs)
    status, rounds, points = (np.empty((P, runs), dtype=int) for _ in range(3))
    xs, pos = [], 0
    for p in range(P):
        dim = probs.dim(p)
        xr = np.empty((runs, dim))
        for r in range(runs):
            status[p, r], rounds[p, r], points[p, r] = np.frombuffer(raw, "<i4", 3, pos)
            pos += 12
            xr[r] = np.frombuffer(raw, "<f8", dim, pos)
            pos += 8 * dim
        xs.append(push_eps(xr))
    assert pos == len(raw)
    spread = np.array([np.abs(xr[1:] - xr[0]).max() / scale_of(xr[0]) if runs > 1 else 0.0 for xr in xs])
    same_path = (status == status[:, :1]).all(axis=1) & (rounds == rounds[:, :1]).all(axis=1)
    stable = same_path & (spread <= SPREAD)
    return Reference(xs, status, rounds, points, stable, spread)


def subset(ref: Reference, idx) -> Reference:
    idx = list(idx)
    return Reference([ref.x[i] for i in idx], ref.status[idx], ref.rounds[idx], ref.points[idx], ref.stable[idx], ref.spread[idx])


def check(name: str, ref: Reference, x, status=None, envelope: bool = False, max_unstable: float = MAX_UNSTABLE):
    """Every stable problem within TOL_STABLE (or a twentieth of its ensemble spread, if larger) of the reference, with
    its status; every unstable one within TOL_UNSTABLE (or the ensemble's own scatter, if larger) of one run of the
    ensemble; at most max_unstable of the problems unstable.  ``envelope``: runs to convergence, whose last iterations
    work at the solver's noise floor -- an unstable problem within 1e-8 or twice the scatter, and no bound on how many are
    unstable.  Prints the calibration record."""
    x = np.asarray(x, dtype=np.float64)
    P = len(ref.x)
    assert x.shape[0] == P
    err = np.array([np.abs(x[p] - ref.x[p][0]).max() / scale_of(ref.x[p][0]) for p in range(P)])
    near = np.array([min(np.abs(x[p] - xr).max() for xr in ref.x[p]) / scale_of(ref.x[p][0]) for p in range(P)])
    st = ref.stable
    tol = np.maximum(TOL_STABLE, ref.spread / 20)
    tol_un = np.maximum(10 * TOL_UNSTABLE, 2 * ref.spread) if envelope else np.maximum(TOL_UNSTABLE, ref.spread)
    n_unst = int((~st).sum())
    e_st = float(err[st].max()) if st.any() else 0.0
    e_un = float(near[~st].max()) if n_unst else 0.0
    print(
        f"[{name}] problems {P}, unstable {n_unst} ({n_unst / P:.1%}); stable: max err {e_st:.2e} "
        f"(max err / tol {float((err / tol)[st].max()) if st.any() else 0:.2f}); unstable: max err to the nearest run {e_un:.2e}"
    )
    bad = np.flatnonzero(st & (err > tol))
    assert bad.size == 0, f"{name}: {bad.size} stable problems off the reference, e.g. #{bad[0]} err {err[bad[0]]:.3e}"
    if status is not None:
        status = np.asarray(status)
        bad = np.flatnonzero(st & (status != ref.status[:, 0]))
        assert bad.size == 0, f"{name}: {bad.size} stable problems end with another status, e.g. #{bad[0]}: {status[bad[0]]} vs {ref.status[bad[0], 0]}"
    bad = np.flatnonzero(~st & (near > tol_un))
    assert bad.size == 0, f"{name}: {bad.size} unstable problems match no run of the ensemble, e.g. #{bad[0]} err {near[bad[0]]:.3e}"
    if not envelope:
        assert n_unst <= max_unstable * P, f"{name}: {n_unst} of {P} problems unstable"
    return err, near
