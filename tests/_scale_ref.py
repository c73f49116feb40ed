"""Cases of the pending exposure scale (``tests/test_gpu_pending_scale.py``, checked on the host by ``test_scale_ref_host.py``).

After ``Engine.set_H_scale`` and after every accepted MvNMF trial the engine does not rewrite H: H is *to be read as*
``clip(H * scale, EPSILON)`` until a pass writes it in full.  A reader that forgets the scale, applies it twice or drops
it gives a finite, plausible, wrong result.  The cases here are built so that each such miss is orders of magnitude
outside every tolerance in use:

* the state comes from ``oracle.klnmf_oracle.floor_state``: a share of H0 sits exactly at EPSILON;
* the scale has entries of ``2.0**-30`` (whole columns of ordinary exposures go below the floor: the clip matters), an
  entry >= 2 (floor entries leave the floor), the rest from ``uniform(0.2, 3.0)`` with nothing within 10 % of 1;
* three conditions hold per case (``Case.conditions``) and are asserted on the host: at least 5 % of ``H0 * scale`` lies
  below EPSILON before the clip, at least 5 % of H0's floor entries leave the floor, and the oracle's objectives of the
  materialised state, of the unscaled state and of the twice-scaled state differ pairwise by more than 1 %.

With one signature the scale has one entry: the shape comes as two cases, ``down`` (``2.0**-30``) and ``up`` (2.5), a tenth
of its exposures is put on the floor by hand (one signature cannot reach it by the update), and the first condition is
asked of ``down``, the second of ``up``.

The MvNMF states (``mv_case``): one whose first line-search trial is accepted and one that backtracks (low counts, a
dominant volume penalty), each with the oracle's gamma.
"""

from __future__ import annotations

import functools
from dataclasses import dataclass

import numpy as np

from oracle import klnmf_oracle as orc

EPS = orc.EPSILON
TINY = 2.0**-30

# (V, N, K): the smallest shapes that reach each branch; N ragged everywhere
SHAPES = [
    (96, 39, 7),      # two full tiles + 7; the small-cohort kernel when on
    (83, 39, 1),      # the scale's padding, masked features
    (96, 1031, 16),   # one tile past the small-cohort limit of 64 tiles: the fused path at a K the small kernel would take
    (96, 215, 17),    # KR != 0 geometry
    (96, 215, 50),
    (96, 215, 64),    # KP == K: no pad column
    (288, 215, 12),   # feature blocks
    (97, 215, 12),    # last block one feature wide
]
# a cooperative leftover tile exists without a scale: kl_step(1), update_W, kl_step_objective only
COOP_SHAPE = (96, 16400, 50)
SMALL_SHAPES = [(96, 39, 7), (83, 39, 1)]  # the one-workgroup kernel takes these (K <= 16, at most 64 tiles)


def active_for(K):
    """As ``test_gpu_floor.active_for``: up to four active signatures per sample, fewer at small K."""
    return (1, max(1, min(4, K // 4)))


def make_scale(K, seed, variant="both"):
    """The scale of a case: ``max(1, K // 8)`` entries of 2**-30, one in [2, 3], the rest from uniform(0.2, 3.0) outside
    [0.9, 1.1].  K = 1: ``down`` is 2**-30, ``up`` is 2.5."""
    rng = np.random.default_rng(seed)
    if K == 1:
        return np.array([TINY if variant == "down" else 2.5])
    s = rng.uniform(0.2, 3.0, K)
    near = np.abs(s - 1.0) <= 0.1
    while near.any():
        s[near] = rng.uniform(0.2, 3.0, int(near.sum()))
        near = np.abs(s - 1.0) <= 0.1
    cols = rng.permutation(K)
    n_tiny = max(1, K // 8)
    s[cols[:n_tiny]] = TINY
    s[cols[n_tiny]] = rng.uniform(2.0, 3.0)
    return s


def materialise(H, scale):
    """What a pending scale means: ``clip(H * scale, EPSILON)`` in float64, one multiplication and one comparison per entry."""
    return np.clip(H * scale[None, :], EPS, None)


def compose(H, *scales):
    """``set_H_scale(s1); set_H_scale(s2)``: the earlier scale is materialised before the next one is taken."""
    for s in scales:
        H = materialise(H, s)
    return H


@dataclass(frozen=True)
class Case:
    V: int
    N: int
    K: int
    variant: str
    X: np.ndarray
    W: np.ndarray
    H0: np.ndarray
    scale: np.ndarray
    scale2: np.ndarray  # a second scale, for the composition
    Hs: np.ndarray

    @property
    def tag(self):
        return f"{self.V}x{self.N}x{self.K}" + ("" if self.variant == "both" else f"-{self.variant}")

    def conditions(self):
        """``(clipped, lifted, (f_materialised, f_unscaled, f_twice))``: the share of ``H0 * scale`` below EPSILON before the
        clip, the share of H0's floor entries that leave the floor, and the oracle's three objectives."""
        raw = self.H0 * self.scale[None, :]
        floor = self.H0 == EPS
        clipped = float(np.mean(raw < EPS))
        lifted = float(np.mean(self.Hs[floor] > EPS)) if floor.any() else 0.0
        Xt, Wt = self.X.T, self.W.T
        f = tuple(orc.kl_divergence(Xt, Wt, H.T) for H in (self.Hs, self.H0, materialise(self.Hs, self.scale)))
        return clipped, lifted, f


def separation(f):
    """The smallest pairwise relative difference of the three objectives."""
    return min(abs(a - b) / max(abs(a), abs(b)) for i, a in enumerate(f) for b in f[i + 1 :])


@functools.lru_cache(maxsize=None)
def case(V, N, K, variant="both"):
    seed = 1000 + V + N + K
    X, W, H0 = orc.floor_state(V, N, K, seed, steps=40, active=active_for(K))
    if K == 1:
        H0 = H0.copy()
        H0[np.random.default_rng(seed).permutation(N)[: max(2, N // 10)], 0] = EPS
    scale = make_scale(K, seed, variant)
    scale2 = make_scale(K, seed + 1, "up" if variant == "down" else "down" if variant == "up" else "both")
    for a in (X, W, H0, scale, scale2):
        a.setflags(write=False)
    Hs = materialise(H0, scale)
    Hs.setflags(write=False)
    return Case(V, N, K, variant, X, W, H0, scale, scale2, Hs)


def variants(K):
    return ("down", "up") if K == 1 else ("both",)


def all_cases(shapes=None):
    """``(V, N, K, variant)`` of every case of ``shapes`` (default: ``SHAPES``)."""
    return [(V, N, K, v) for V, N, K in (SHAPES if shapes is None else shapes) for v in variants(K)]


def case_id(p):
    return f"{p[0]}x{p[1]}x{p[2]}" + ("" if p[3] == "both" else f"-{p[3]}")


# ------------------------------------------------------------------ MvNMF: the pending state an accepted trial leaves


@dataclass(frozen=True)
class MvCase:
    name: str
    X: np.ndarray
    W: np.ndarray
    H: np.ndarray
    lam: float
    delta: float
    n_given: int
    gamma: float  # the oracle's gamma after one step from gamma = 1
    Wn: np.ndarray  # the oracle's state after that step (sample-major)
    Hn: np.ndarray

    @property
    def backtracks(self):
        return self.gamma < 1.0  # one rejected trial: 0.8 * 1.2 = 0.96; an accepted first trial: min(1, 1.2) = 1

    @property
    def shape(self):
        return self.X.shape[1], self.X.shape[0], self.W.shape[0]


MV_CASES = ("accepted", "accepted-given2", "backtracking", "accepted-65x96", "accepted-65x192")
MV_NARROW = MV_CASES[:3]  # one feature block, at most 64 signatures: the pending state survives the step
MV_CHUNKED = MV_CASES[3:]  # K = 65: the line search flushes at once (``if (e->NC > 1) flush_H_scale``)


@functools.lru_cache(maxsize=None)
def mv_case(name):
    """``accepted*``: a floor state, lam = delta = 1.  ``backtracking``: ``test_wide_many_mvnmf_backtracking`` scaled down to one
    feature block and 50 signatures (mean 100 mutations per sample, lam = 1e4): the state before the first oracle step
    that rejects its first trial."""
    if name == "backtracking":
        V, N, K, lam, delta, g = 96, 215, 50, 1.0e4, 1.0, 0
        X, W, H = orc.synthetic_problem(V, N, K, seed=77, mean_mutations=100.0)
        X = X.clip(EPS)
        Wt, Ht = W.T, H.T
        for _ in range(12):
            Wn, Hn, gamma = orc.mvnmf_step(X.T, Wt, Ht, lam, delta, 1.0, g)
            if gamma < 1.0:
                break
            Wt, Ht = Wn, Hn
    else:
        V, N, K, g = {"accepted": (96, 215, 17, 0), "accepted-given2": (96, 215, 12, 2), "accepted-65x96": (96, 215, 65, 0),
                      "accepted-65x192": (192, 215, 65, 0)}[name]
        lam, delta = 1.0, 1.0
        X, W, H = orc.floor_state(V, N, K, 2000 + V + K, steps=40, active=active_for(K), n_given=g)
        Wt, Ht = W.T, H.T
        Wn, Hn, gamma = orc.mvnmf_step(X.T, Wt, Ht, lam, delta, 1.0, g)
    out = [np.ascontiguousarray(a) for a in (X, Wt.T, Ht.T, Wn.T, Hn.T)]
    for a in out:
        a.setflags(write=False)
    return MvCase(name, out[0], out[1], out[2], lam, delta, g, float(gamma), out[3], out[4])
