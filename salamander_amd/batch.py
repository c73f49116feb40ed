"""Python handle of one device batch: many KLNMF models of at most 16 signatures on one count matrix (``KLNMFSweep``).

Thin, in the style of ``engine.py``: validates shapes, hands plain pointers to the ``salnmf_batch_*`` entry points of
``include/salnmf.h`` and turns status codes into exceptions.  Members are numbered in the order of ``n_signatures``;
arrays are in AnnData's storage layout (``X (N, V)``, ``W (K, V)``, ``H (N, K)``, float64, C order).
"""

from __future__ import annotations

import ctypes
from ctypes import POINTER, c_double, c_int

import numpy as np

from . import _lib
from .engine import _as_c, _ptr
from .resample import check_n_resamples, check_seed
from .split import check_n_splits, heldout_scale, train_threshold
from .stability import _Outputs, check_errors, check_group_shape, check_max_rounds

SLOTS = _lib.BATCH_SLOTS
MAX_SAMPLES = 1024  # 64 tiles of 16 samples (the small-cohort kernel's reach)
MAX_FEATURES = 96
MAX_SIGNATURES = 16


def _ints(values) -> np.ndarray:
    return np.ascontiguousarray(np.asarray(values, dtype=np.int32).reshape(-1))


def _iptr(a):
    return a.ctypes.data_as(POINTER(c_int))


class BatchEngine:
    """Device-resident state of a sweep: X once, bootstrap resamples of it on request, W / H / numerator per member."""

    def __init__(self, n_samples: int, n_features: int, n_signatures, device: int = 0):
        self._lib = _lib.load()
        if self._lib.salnmf_device_count() < 1:
            raise _lib.EngineUnavailable(
                "no HIP device visible: salamander_amd runs on MI355X (gfx950) only and has no CPU fallback."
            )
        self.N, self.V, self.device = int(n_samples), int(n_features), int(device)
        self.Ks = [int(k) for k in n_signatures]
        self.M = len(self.Ks)
        ks = _ints(self.Ks)
        handle = ctypes.c_void_p()
        _lib.check(self._lib.salnmf_batch_create(self.device, self.V, self.N, self.M, _iptr(ks), ctypes.byref(handle)))
        self._handle = handle
        self.R = 0  # resamples of X on the device
        self.F = 0  # count splits of X on the device (datasets 0 .. F - 1 train, F .. 2 F - 1 test)

    @property
    def _h(self):
        h = getattr(self, "_handle", None)
        if not h:
            raise RuntimeError("salnmf: this BatchEngine has been closed")
        return h

    def close(self):
        if getattr(self, "_handle", None):
            self._lib.salnmf_batch_destroy(self._handle)
            self._handle = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def upload_X(self, X, clip: bool = False):
        X = _as_c(X, (self.N, self.V), "X")
        _lib.check(self._lib.salnmf_batch_upload_X(self._h, _ptr(X), int(bool(clip))))
        self.R = self.F = 0  # (the resamples and splits go with the X they were drawn from)

    def resample(self, n_resamples: int, seed: int = 0):
        """Draw ``n_resamples`` bootstrap resamples of the uploaded X on the device (``resample.py``): datasets
        ``0 .. n_resamples - 1`` of this batch, dataset -1 being X itself.  Every member is back on dataset -1."""
        R, seed = check_n_resamples(n_resamples), check_seed(seed)
        self.R = 0
        _lib.check(self._lib.salnmf_batch_resample(self._h, R, seed))
        self.R = R

    def split(self, n_splits: int, train_fraction: float = 0.5, seed: int = 0):
        """Draw ``n_splits`` count splits of the uploaded X on the device (``split.py``): train split f is dataset f, test
        split f dataset ``n_splits + f``, dataset -1 being X itself.  Every member is back on dataset -1.  A batch holds
        splits or resamples, not both."""
        F, thr, seed = check_n_splits(n_splits), train_threshold(train_fraction), check_seed(seed)
        _lib.check(self._lib.salnmf_batch_split(self._h, F, thr, seed))
        self.F, self.R = F, 0

    def heldout_kl(self, members, datasets, train_fraction: float = 0.5) -> np.ndarray:
        """Per-sample KL divergences of ``members[i]`` against dataset ``datasets[i]`` instead of its own, its exposures
        scaled by ``(1 - train_fraction) / train_fraction`` and clipped: ``(len(members), N)``.  The members keep their
        datasets."""
        train_threshold(train_fraction)
        m, d = _ints(members), _ints(datasets)
        if m.shape != d.shape:
            raise ValueError("'members' and 'datasets' must have the same length.")
        out = np.empty((len(m), self.N), dtype=np.float64)
        _lib.check(self._lib.salnmf_batch_heldout_kl(self._h, len(m), _iptr(m), _iptr(d), heldout_scale(train_fraction), _ptr(out)))
        return out

    def profile_split(self, n_splits: int, train_fraction: float = 0.5, seed: int = 0, n_calls: int = 20) -> float:
        """Development aid: average milliseconds of the split kernel alone, by device events."""
        ms = c_double(0.0)
        F, thr = check_n_splits(n_splits), train_threshold(train_fraction)
        _lib.check(self._lib.salnmf_profile_split(self._h, F, thr, check_seed(seed), int(n_calls), ctypes.byref(ms)))
        self.F, self.R = F, 0
        return float(ms.value)

    def set_dataset(self, member: int, dataset: int):
        """The matrix ``member`` fits from now on: resample (or split half) ``dataset``, or -1 for the uploaded X (the default)."""
        _lib.check(self._lib.salnmf_batch_set_dataset(self._h, int(member), int(dataset)))

    def download_dataset(self, dataset: int, raw: bool = False) -> np.ndarray:
        """A dataset as ``(N, V)`` -- a resample as plain counts, dataset -1 as the device holds it -- or, with ``raw``,
        the slot as the kernels read it: ``(16 * ceil(N / 16), 96)``, padded with zeros, entries clipped to EPSILON."""
        shape = (16 * ((self.N + 15) // 16), MAX_FEATURES) if raw else (self.N, self.V)
        out = np.empty(shape, dtype=np.float64)
        _lib.check(self._lib.salnmf_batch_download_dataset(self._h, int(dataset), int(bool(raw)), _ptr(out)))
        return out

    def profile_resample(self, n_resamples: int, seed: int = 0, n_calls: int = 20) -> float:
        """Development aid: average milliseconds of the resample kernel alone, by device events."""
        ms = c_double(0.0)
        _lib.check(self._lib.salnmf_profile_resample(self._h, check_n_resamples(n_resamples), check_seed(seed), int(n_calls), ctypes.byref(ms)))
        self.R = int(n_resamples)
        return float(ms.value)

    def upload_member(self, member: int, W, H):
        K = self.Ks[member]
        W = _as_c(W, (K, self.V), "W")
        H = _as_c(H, (self.N, K), "H")
        _lib.check(self._lib.salnmf_batch_upload_member(self._h, int(member), _ptr(W), _ptr(H)))

    def download_member(self, member: int):
        """``(W, H)`` of one member."""
        K = self.Ks[member]
        W = np.empty((K, self.V), dtype=np.float64)
        H = np.empty((self.N, K), dtype=np.float64)
        _lib.check(self._lib.salnmf_batch_download_member(self._h, int(member), _ptr(W), _ptr(H)))
        return W, H

    def set_weights(self, member: int, weights_kl=None, weights_lhalf=None):
        """Per-sample weights of one member, as ``Engine.set_weights``: ``(N,)`` arrays or None; None / None clears them.
        Finite, non-negative entries only.  The member's steps and queued objectives are then the weighted ones;
        ``samplewise_kl`` and ``heldout_kl`` stay unweighted."""
        wk = None if weights_kl is None else _as_c(weights_kl, (self.N,), "weights_kl")
        wl = None if weights_lhalf is None else _as_c(weights_lhalf, (self.N,), "weights_lhalf")
        _lib.check(self._lib.salnmf_batch_set_weights(self._h, int(member), None if wk is None else _ptr(wk), None if wl is None else _ptr(wl)))

    def kl_step(self, n_steps: int, members, n_given):
        """``n_steps`` joint updates of each listed member (``n_given[i]`` given signatures of ``members[i]``)."""
        m, g = _ints(members), _ints(n_given)
        if m.shape != g.shape:
            raise ValueError("'members' and 'n_given' must have the same length.")
        _lib.check(self._lib.salnmf_batch_kl_step(self._h, int(n_steps), len(m), _iptr(m), _iptr(g)))

    def objective_async(self, slot: int, members):
        """Queue the objectives of the listed members into row ``slot`` of the objective array (no host round trip)."""
        m = _ints(members)
        _lib.check(self._lib.salnmf_batch_objective_async(self._h, int(slot), len(m), _iptr(m)))

    def objective_read(self, first: int, count: int) -> np.ndarray:
        """Rows ``[first, first + count)`` of the objective array: ``(count, n_members)``."""
        out = np.empty((int(count), self.M), dtype=np.float64)
        _lib.check(self._lib.salnmf_batch_objective_read(self._h, int(first), int(count), out.ctypes.data_as(POINTER(c_double))))
        return out

    def samplewise_kl(self) -> np.ndarray:
        """Per-sample KL divergences of every member: ``(n_members, N)``."""
        out = np.empty((self.M, self.N), dtype=np.float64)
        _lib.check(self._lib.salnmf_batch_samplewise_kl(self._h, out.ctypes.data_as(POINTER(c_double))))
        return out

    def stability(self, groups, errors=None, max_rounds: int = 20):
        """Match, cluster and score the signatures of the listed members where they lie on the device (``stability.py``).

        ``groups`` is a list of lists of member indices, each list of one number of signatures and at least two members;
        ``errors`` one sequence per group with one value per member (None: all zero).  One launch for all groups; returns
        one ``StabilityResult`` per group.  ``ValueError`` before any launch for a group that mixes numbers of signatures
        or has fewer than two members."""
        groups = [[int(m) for m in g] for g in groups]
        max_rounds = check_max_rounds(max_rounds)
        if not groups:
            raise ValueError("'groups' must hold at least one group.")
        shapes = []
        for g in groups:
            if any(not 0 <= m < self.M for m in g):
                raise ValueError(f"A group lists a member outside 0 .. {self.M - 1}.")
            ks = {self.Ks[m] for m in g}
            if len(ks) > 1:
                raise ValueError(f"The members of one group must share their number of signatures, got {sorted(ks)}.")
            check_group_shape(len(g), ks.pop() if ks else 1, self.V)
            shapes.append((len(g), self.Ks[g[0]]))
        errs = check_errors(errors, shapes)
        offsets = _ints(np.concatenate([[0], np.cumsum([len(g) for g in groups])]))
        members = _ints([m for g in groups for m in g])
        out = _Outputs(shapes)
        _lib.check(self._lib.salnmf_batch_stability(
            self._h, len(groups), _iptr(offsets), _iptr(members), None if errs is None else _ptr(errs), max_rounds, *out.pointers(),
        ))
        return out.results(self.V)
