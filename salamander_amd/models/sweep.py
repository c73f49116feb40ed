"""``KLNMFSweep``: many KLNMF fits of one count matrix -- a range of signature counts, several seeds -- in one batched run.

The reference's tutorial chooses the number of signatures by fitting one model per candidate, one after another
(``tutorial.ipynb`` section 1.6)::

    for n_signatures in range(1, 10):
        model = KLNMF(n_signatures=n_signatures); model.fit(adata.copy())

At the tutorial's size (192 samples x 96 features) one fit keeps one CU busy and the rest of the device idle.  The sweep
runs the members side by side instead: one workgroup per model, all of them in each launch (``batch.py``,
``csrc/salnmf_batch.h``).  Every member comes out bit for bit as the fit of the loop above with
``objective_in_step=False``: the same initialisation (``StandardNMF._initialize`` on the member's own model, in member
order), the same steps, objectives and convergence tests.  Members the batched kernel cannot run (more than 16 signatures,
more than 1 024 samples or 96 features, all signatures given) are fitted one after another by ``KLNMF.fit``.

``n_resamples=R`` adds bootstrap resamples of the counts as a third axis: the R matrices are drawn once on the device
(``resample.py``: each sample's mutations redrawn from its own observed spectrum, bit-reproducible from ``resample_seed``),
member (K, seed, r) fits resample r, and every member still equals the single fit on its matrix bit for bit.  What the
field does with such fits -- keep the largest K whose signatures come back the same -- is ``stability=True``: for every K
the signatures of all its members are matched to each other, clustered into consensus signatures and scored by their
silhouettes on the device (``stability.py``), and ``suggest_n_signatures`` applies the customary thresholds.

``n_splits=F`` adds the second criterion, held-out likelihood by count splitting (``split.py``): the counts are thinned F
times on the device into independent train and test halves, member (K, seed, f) fits ``train_splits_[f]`` -- again bit for
bit the single fit on that matrix -- and is scored against ``test_splits_[f]`` with its exposures scaled by
``(1 - p) / p``, all batched members in one launch of the forward pass (``BatchEngine.heldout_kl``).
``suggest_n_signatures_heldout`` returns the K of smallest mean held-out divergence.

``lhalf_weights=[...]`` adds the l-half sparsity penalty as an axis of its own and ``weights_kl`` per-sample KL weights
shared by all members: member (K, penalty, seed, r) is bit for bit the single fit with
``fitting_kwargs={"weights_kl": weights_kl, "weights_lhalf": penalty}``, run in the weighted instantiation of the batched
step (``BatchEngine.set_weights``).  With ``n_splits`` the penalty is chosen like K, by held-out likelihood
(``suggest_penalty_heldout``).
"""

from __future__ import annotations

import time
from typing import Any

import numpy as np

from ..anndata_compat import ANNDATA_TYPES
from ..batch import MAX_FEATURES, MAX_SAMPLES, MAX_SIGNATURES, SLOTS, BatchEngine
from ..initialization import INIT_METHODS, check_given_asignatures
from ..engine import Engine
from ..resample import check_counts, check_n_resamples, check_seed, resample_counts
from ..split import check_n_splits, heldout_scale, split_counts, train_threshold
from ..stability import MAX_FEATURES as STABILITY_MAX_FEATURES
from ..stability import MAX_SIGNATURES as STABILITY_MAX_SIGNATURES
from ..stability import check_max_rounds, signature_stability
from ..utils import EPSILON, type_checker, value_checker
from .klnmf import KLNMF
from .signature_nmf import SignatureNMF


class KLNMFSweep:
    """Fit ``KLNMF(K)`` for every K of ``ns_signatures`` and every seed of ``seeds`` on one count matrix.

    ``fit`` returns the models in K-major, seed-minor order; ``reconstruction_errors_`` holds their summed sample-wise
    KL divergences as ``(len(ns_signatures), max(1, len(seeds)))``, ``batched_`` whether each member ran in the batched
    kernel (True) or through ``KLNMF.fit`` (False).  Hyperparameters are shared by all members.

    With ``n_resamples = R >= 1`` the members are K-major, seed-middle, resample-minor and member (K, seed, r) fits
    ``resamples_[r]``, the r-th bootstrap resample of the counts (the same R matrices for every K and seed, drawn from
    ``resample_seed``).  ``resamples_`` is ``(R, N, V)``, ``resample_of_`` holds r per member (-1 without resamples) and
    ``reconstruction_errors_`` is ``(len(ns_signatures), max(1, len(seeds)), R)``.  The counts must be non-negative
    integer values with row totals below 2**32.

    With ``stability=True`` (every K needs at least two members: seeds x resamples) the members of each K form one group
    whose signatures are matched, clustered and scored after the fits, in one launch over all K, members in sweep order,
    the anchor of a group being its member of smallest summed reconstruction error: ``stability_mean_`` and
    ``stability_min_`` ``(len(ns_signatures),)`` and, one entry per K, ``cluster_stability_ (K,)``,
    ``consensus_signatures_ (K, V)``, ``assignments_ (M, K)``, ``silhouettes_ (M, K)``, ``stability_rounds_`` and
    ``stability_converged_``; ``timings_["stability_s"]`` is the time it took.  A K the kernel cannot take (more than 16
    signatures, or more than 96 features) gets NaN scores, ``None`` for its arrays, 0 rounds and ``False``.
    ``suggest_n_signatures`` picks the largest K that passes the thresholds; it raises ``ValueError`` on a sweep built
    without ``stability=True`` and returns ``None`` before ``fit`` (the scores are NaN until then).

    With ``n_splits = F >= 1`` (not together with ``n_resamples``) the counts are split F times by thinning: every
    mutation goes to ``train_splits_[f]`` with probability ``train_fraction`` and to ``test_splits_[f]`` otherwise (both
    ``(F, N, V)``, drawn from ``split_seed``).  The members are K-major, seed-middle, split-minor, member (K, seed, f) fits
    ``train_splits_[f]``; ``split_of_`` holds f per member (-1 without splits) and ``reconstruction_errors_`` (the training
    error) is ``(len(ns_signatures), max(1, len(seeds)), F)``.  Each model's ``adata.obs["heldout_error"]`` is its
    per-sample KL divergence to ``max(test_splits_[f], EPSILON)`` with the exposures ``max(c H, EPSILON)``,
    ``c = (1 - train_fraction) / train_fraction``; ``heldout_errors_`` holds the sums, shaped like
    ``reconstruction_errors_``.  For every (K, f) the seed of smallest training error (lowest index on ties) is taken --
    nothing of the test half enters the selection -- and ``heldout_mean_`` / ``heldout_sem_`` ``(len(ns_signatures),)``
    are the mean of its held-out error over f and ``std(ddof=1) / sqrt(F)`` (NaN at F = 1).
    ``timings_["split_s"]`` and ``timings_["heldout_s"]`` are the time of the draw and of the scoring.  With
    ``stability=True`` the members of a K count as seeds x splits.

    ``lhalf_weights`` (a non-empty sequence of L finite, non-negative floats; not together with ``stability=True``) adds a
    penalty axis: the members are K-major, then penalty, then seed, then resample / split minor, ``lhalf_of_`` holds the
    penalty index per member (-1 without the axis), ``reconstruction_errors_`` and ``heldout_errors_`` are
    ``(len(ns_signatures), L, seeds[, R or F])`` and ``heldout_mean_`` / ``heldout_sem_`` ``(len(ns_signatures), L)``, the
    seed of smallest training error being taken per (K, penalty, f).  A penalty of 0.0 is the penalised closed form at zero
    weight -- what a single fit with ``weights_lhalf=0.0`` runs -- not the unpenalised member.  ``weights_kl`` (a scalar,
    list or ``(n_obs,)`` array, validated at ``fit`` as a single fit validates it) is shared by all members and allowed
    without the axis.  Held-out scoring stays unweighted.  Without either, every attribute, shape and member order is as
    above."""

    def __init__(
        self,
        ns_signatures=range(1, 10),
        seeds=None,
        init_method: str = "nndsvd",
        min_iterations: int = 500,
        max_iterations: int = 10000,
        conv_test_freq: int = 10,
        tol: float = 1e-7,
        device: int = 0,
        device_init: bool = True,
        distributed: bool = False,
        n_resamples: int = 0,
        resample_seed: int = 0,
        stability: bool = False,
        stability_max_rounds: int = 20,
        n_splits: int = 0,
        train_fraction: float = 0.5,
        split_seed: int = 0,
        lhalf_weights=None,
        weights_kl=None,
    ):
        ns = list(ns_signatures)
        if not ns or not all(isinstance(k, (int, np.integer)) and not isinstance(k, bool) and k > 0 for k in ns):
            raise ValueError("'ns_signatures' must be a non-empty collection of positive integers.")
        if distributed:
            raise ValueError("A sweep runs on one device: 'distributed=True' is not supported.")
        value_checker("init_method", init_method, INIT_METHODS)
        self.n_resamples = check_n_resamples(n_resamples, minimum=0)
        self.resample_seed = check_seed(resample_seed)
        self.n_splits = check_n_splits(n_splits, minimum=0)
        train_threshold(train_fraction)
        self.train_fraction = float(train_fraction)
        self.split_seed = check_seed(split_seed)
        if self.n_splits and self.n_resamples:
            raise ValueError("'n_splits' and 'n_resamples' exclude each other: a sweep fits count splits or bootstrap resamples, not both.")
        self.ns_signatures = [int(k) for k in ns]
        self.seeds = None if not seeds else [int(s) for s in seeds]
        self.stability = bool(stability)
        self.stability_max_rounds = check_max_rounds(stability_max_rounds)
        if self.stability and max(1, len(self.seeds or [])) * max(1, self.n_resamples) * max(1, self.n_splits) < 2:
            raise ValueError("'stability=True' needs at least two members per number of signatures: several seeds, or n_resamples >= 2.")
        if lhalf_weights is not None:
            try:
                penalties = [float(v) for v in lhalf_weights]
            except TypeError:
                raise ValueError("'lhalf_weights' must be a non-empty sequence of finite, non-negative floats.") from None
            if not penalties or not all(np.isfinite(v) and v >= 0.0 for v in penalties):
                raise ValueError("'lhalf_weights' must be a non-empty sequence of finite, non-negative floats.")
            if self.stability:
                raise ValueError("'stability=True' is not supported together with 'lhalf_weights': grouping per (K, penalty) is not built.")
            self.lhalf_weights = penalties
        else:
            self.lhalf_weights = None
        self.weights_kl = weights_kl
        self.init_method = init_method
        self.min_iterations = min_iterations
        self.max_iterations = max_iterations
        self.conv_test_freq = conv_test_freq
        self.tol = tol
        self.device = device
        self.device_init = device_init
        self.models_: list[KLNMF] = []
        self.batched_ = np.zeros(0, dtype=bool)
        self.reconstruction_errors_ = np.zeros((0, 0))
        self.resamples_ = None
        self.resample_of_ = np.zeros(0, dtype=int)
        self.train_splits_ = None
        self.test_splits_ = None
        self.split_of_ = np.zeros(0, dtype=int)
        self.lhalf_of_ = np.zeros(0, dtype=int)
        self.heldout_errors_ = np.zeros((0, 0, 0))
        summary = (len(self.ns_signatures), len(self.lhalf_weights)) if self.lhalf_weights else len(self.ns_signatures)
        self.heldout_mean_ = np.full(summary, np.nan)
        self.heldout_sem_ = np.full(summary, np.nan)
        self._fitted = False
        self.timings_: dict[str, float] = {}
        self.member_steps_ = 0
        self._clear_stability()

    # ------------------------------------------------------------------ members
    def _model(self, n_signatures: int) -> KLNMF:
        return KLNMF(
            n_signatures, self.init_method, self.min_iterations, self.max_iterations, self.conv_test_freq, self.tol,
            objective_in_step=False, device=self.device, device_init=self.device_init,
        )

    def _members(self, init_kwargs):
        """``(K, init_kwargs of the member, resample or split of the member or -1, penalty index or -1)`` in K-major, then
        penalty, then seed, then resample-minor (split-minor) order."""
        base = {} if init_kwargs is None else dict(init_kwargs)
        resamples = range(self.n_resamples) if self.n_resamples else range(self.n_splits) if self.n_splits else [-1]
        out = []
        penalties = range(len(self.lhalf_weights)) if self.lhalf_weights else [-1]
        for k in self.ns_signatures:
            for l in penalties:
                for kwargs in [base | {"seed": s} for s in self.seeds] if self.seeds else [init_kwargs]:
                    out.extend((k, kwargs, r, l) for r in resamples)
        return out

    def _fitting_kwargs(self, l: int):
        """The ``fitting_kwargs`` of the single fit a member equals: None without weights, as today."""
        if l < 0 and self.weights_kl is None:
            return None
        return {"weights_kl": self.weights_kl, "weights_lhalf": self.lhalf_weights[l] if l >= 0 else None}

    def _member_adata(self, adata, r: int):
        """The member's own copy of the data: the caller's, or resample r (train split r) under the caller's obs / var names."""
        own = adata.copy()
        if r >= 0:
            own.X = (self.train_splits_ if self.n_splits else self.resamples_)[r].copy()
        return own

    @staticmethod
    def _close_engine(model: KLNMF) -> None:
        if model._engine is not None:
            model._engine.close()
            model._engine = None
        model._resident = set()

    # ------------------------------------------------------------------ stability
    def _clear_stability(self) -> None:
        n = len(self.ns_signatures)
        self.stability_mean_ = np.full(n, np.nan)
        self.stability_min_ = np.full(n, np.nan)
        self.cluster_stability_ = [None] * n
        self.consensus_signatures_ = [None] * n
        self.assignments_ = [None] * n
        self.silhouettes_ = [None] * n
        self.stability_rounds_ = np.zeros(n, dtype=int)
        self.stability_converged_ = np.zeros(n, dtype=bool)

    def _run_stability(self, batch, slot_of, members, models, n_vars: int) -> None:
        """One group per entry of ``ns_signatures`` (its members in sweep order), all groups in one launch: in place on the
        batch when every member of every group lies there, else stand-alone on the models' signatures."""
        per_k = len(members) // len(self.ns_signatures)
        groups = [list(range(g * per_k, (g + 1) * per_k)) for g in range(len(self.ns_signatures))]
        taken = [g for g, k in enumerate(self.ns_signatures) if k <= STABILITY_MAX_SIGNATURES and n_vars <= STABILITY_MAX_FEATURES]
        if not taken:
            return
        errors = [[models[i].reconstruction_error for i in groups[g]] for g in taken]
        if batch is not None and all(i in slot_of for g in taken for i in groups[g]):
            results = batch.stability([[slot_of[i] for i in groups[g]] for g in taken], errors, self.stability_max_rounds)
        else:
            signatures = [np.stack([np.asarray(models[i].asignatures.X, dtype=np.float64) for i in groups[g]]) for g in taken]
            results = signature_stability(signatures, errors, self.stability_max_rounds, device=self.device)
        for g, res in zip(taken, results):
            self.stability_mean_[g], self.stability_min_[g] = res.stability_mean, res.stability_min
            self.cluster_stability_[g] = res.cluster_stability
            self.consensus_signatures_[g] = res.consensus
            self.assignments_[g] = res.assignments
            self.silhouettes_[g] = res.silhouette
            self.stability_rounds_[g], self.stability_converged_[g] = res.n_rounds, res.converged

    def suggest_n_signatures(self, mean_stability: float = 0.8, min_stability: float = 0.2):
        """The largest K of ``ns_signatures`` whose ``stability_mean_`` is at least ``mean_stability`` and whose
        ``stability_min_`` is at least ``min_stability`` (the field's customary thresholds), or None if there is none."""
        if not self.stability:
            raise ValueError("'suggest_n_signatures' needs a sweep fitted with 'stability=True'.")
        ok = [k for k, a, b in zip(self.ns_signatures, self.stability_mean_, self.stability_min_) if a >= mean_stability and b >= min_stability]
        return max(ok) if ok else None

    # ------------------------------------------------------------------ held-out likelihood
    def _heldout_single(self, model: KLNMF, f: int) -> np.ndarray:
        """A fallback member's per-sample held-out divergences: one engine on the clipped test half with the model's
        signatures and its scaled, clipped exposures.  For a shape the batch reaches, the bits ``BatchEngine.heldout_kl``
        gives."""
        eps = float(EPSILON)
        X = np.maximum(self.test_splits_[f], eps)
        H = np.maximum(heldout_scale(self.train_fraction) * np.asarray(model.adata.obsm["exposures"], dtype=np.float64), eps)
        n_obs, n_vars = X.shape
        engine = Engine(n_obs, n_vars, model.n_signatures, device=self.device)
        try:
            engine.upload_X(X)
            engine.upload_W(np.asarray(model.asignatures.X, dtype=np.float64))
            engine.upload_H(H)
            return np.asarray(engine.samplewise_kl(), dtype=np.float64)
        finally:
            engine.close()

    def _summarise_heldout(self, train_errors: np.ndarray, heldout_errors: np.ndarray) -> None:
        """``heldout_mean_`` / ``heldout_sem_`` from ``(len(ns), [L,] seeds, F)`` training and held-out errors: per (K, f)
        -- per (K, penalty, f) -- the seed of smallest training error, lowest index on ties."""
        F = heldout_errors.shape[-1]
        best = np.argmin(train_errors, axis=-2)  # (the first of equal minima)
        chosen = np.take_along_axis(heldout_errors, best[..., None, :], axis=-2)[..., 0, :]
        self.heldout_mean_ = chosen.mean(axis=-1)
        self.heldout_sem_ = chosen.std(axis=-1, ddof=1) / np.sqrt(F) if F > 1 else np.full(chosen.shape[:-1], np.nan)

    def suggest_n_signatures_heldout(self, one_standard_error: bool = False):
        """The K of ``ns_signatures`` with the smallest ``heldout_mean_`` (the first of equal ones); with
        ``one_standard_error`` the smallest K whose mean is at most that minimum plus the minimum's ``heldout_sem_`` (the
        customary rule; with a NaN standard error, at F = 1, the minimiser itself).  None before ``fit``.  On a sweep with
        ``lhalf_weights`` the K of ``suggest_penalty_heldout``'s pair."""
        if not self.n_splits:
            raise ValueError("'suggest_n_signatures_heldout' needs a sweep built with 'n_splits' > 0.")
        if not self._fitted:
            return None
        if self.lhalf_weights:
            return self.suggest_penalty_heldout(one_standard_error)[0]
        best = int(np.nanargmin(self.heldout_mean_))
        if not one_standard_error or np.isnan(self.heldout_sem_[best]):
            return self.ns_signatures[best]
        bound = self.heldout_mean_[best] + self.heldout_sem_[best]
        return min(k for k, mean in zip(self.ns_signatures, self.heldout_mean_) if mean <= bound)

    def suggest_penalty_heldout(self, one_standard_error: bool = False):
        """``(K, penalty)`` of the smallest ``heldout_mean_`` (the first of equal ones, K-major); with
        ``one_standard_error``, among the cells whose mean is at most that minimum plus the minimum's ``heldout_sem_``, the
        smallest K and then the largest penalty (the sparsest model the data cannot tell from the best; with a NaN standard
        error, at F = 1, the minimiser itself).  None before ``fit``.

        The penalty returned is the value fitted on TRAINING halves, which hold a fraction p = ``train_fraction`` of the
        mutations.  The KL term scales with p and the l-half penalty with sqrt(p), so the same trade-off on the full
        counts is ``penalty / sqrt(p)``."""
        if not self.n_splits or not self.lhalf_weights:
            raise ValueError("'suggest_penalty_heldout' needs a sweep built with 'lhalf_weights' and 'n_splits' > 0.")
        if not self._fitted:
            return None
        mean, sem = np.asarray(self.heldout_mean_), np.asarray(self.heldout_sem_)
        bk, bl = np.unravel_index(int(np.nanargmin(mean)), mean.shape)
        if not one_standard_error or np.isnan(sem[bk, bl]):
            return self.ns_signatures[bk], self.lhalf_weights[bl]
        bound = mean[bk, bl] + sem[bk, bl]
        cells = [(self.ns_signatures[i], self.lhalf_weights[j]) for i in range(mean.shape[0]) for j in range(mean.shape[1]) if mean[i, j] <= bound]
        return min(cells, key=lambda c: (c[0], -c[1]))

    # ------------------------------------------------------------------ resamples and splits
    def _draw_datasets(self, batch, counts, slot_of, members) -> float:
        """The R resamples or the F splits, once: drawn into the batch's own slots (resample r is its dataset r; train split
        f its dataset f, test split f its dataset F + f) with every batched member pointed at its own, or stand-alone when
        there is no batch.  Sets ``resamples_``, or ``train_splits_`` and ``test_splits_``; returns the seconds it took."""
        ta = time.perf_counter()
        R, F = self.n_resamples, self.n_splits
        n = R or F
        if batch is not None:
            if R:
                batch.resample(R, self.resample_seed)
            else:
                batch.split(F, self.train_fraction, self.split_seed)
            drawn = [np.stack([batch.download_dataset(first + d) for d in range(n)]) for first in ([0] if R else [0, F])]
            for i, j in slot_of.items():
                batch.set_dataset(j, members[i][2])
        elif R:
            drawn = [resample_counts(counts, R, self.resample_seed, device=self.device)]
        else:
            drawn = split_counts(counts, F, self.train_fraction, self.split_seed, device=self.device)
        if R:
            self.resamples_ = drawn[0]
        else:
            self.train_splits_, self.test_splits_ = drawn
        return time.perf_counter() - ta

    # ------------------------------------------------------------------ fit
    def fit(self, adata, given_parameters: dict[str, Any] | None = None, init_kwargs: dict[str, Any] | None = None,
            fitting_kwargs: dict[str, Any] | None = None, history: bool = True) -> list[KLNMF]:
        type_checker("adata", adata, ANNDATA_TYPES)
        if fitting_kwargs and (set(fitting_kwargs) - {"weights_kl", "weights_lhalf"} or any(v is not None for v in fitting_kwargs.values())):
            raise ValueError("A sweep takes no 'fitting_kwargs': its weighted step is set up by the constructor ('weights_kl' for all members, 'lhalf_weights' as a penalty axis).")
        n_given = SignatureNMF._n_given(given_parameters)
        if given_parameters and "asignatures" in given_parameters:
            for k in self.ns_signatures:  # (KLNMF.fit's own check, before any member is touched)
                check_given_asignatures(given_parameters["asignatures"], adata, k)
        n_obs, n_vars = np.shape(adata.X)
        R, F = self.n_resamples, self.n_splits
        counts = check_counts(adata.X) if R or F else None  # (before anything touches the device)
        if self.weights_kl is not None:  # (a single fit's own check and exceptions, before any member is touched)
            probe = self._model(self.ns_signatures[0])
            probe.adata = adata
            probe._weight_vector("weights_kl", self.weights_kl)
        members = self._members(init_kwargs)
        in_reach = [n_obs <= MAX_SAMPLES and n_vars <= MAX_FEATURES and k <= MAX_SIGNATURES and k > n_given for k, _, _, _ in members]

        t0 = time.perf_counter()
        batch_ids = [i for i, ok in enumerate(in_reach) if ok]
        batch = None
        if batch_ids:
            try:
                batch = BatchEngine(n_obs, n_vars, [members[i][0] for i in batch_ids], device=self.device)
            except RuntimeError:
                batch = None  # (a device without the batched kernel: every member takes KLNMF.fit)
        slot_of = {i: j for j, i in enumerate(batch_ids)} if batch is not None else {}
        models: list[KLNMF] = []
        t_init = t_fallback = t_draw = t_stability = t_heldout = 0.0
        self.resamples_ = self.train_splits_ = self.test_splits_ = None
        self._clear_stability()
        try:
            if batch is not None:
                batch.upload_X(np.asarray(adata.X, dtype=np.float64), clip=True)
            if R or F:
                t_draw = self._draw_datasets(batch, counts, slot_of, members)
            # every member in order: initialised (batched) or fitted (fallback) exactly as the tutorial's loop would
            # do it, so that the legacy NumPy RNG of the random methods advances the same way
            for i, (k, kwargs, r, l) in enumerate(members):
                model = self._model(k)
                fitting = self._fitting_kwargs(l)
                ta = time.perf_counter()
                if i in slot_of:
                    model._setup_adata(self._member_adata(adata, r))  # (the member's own copy, X clipped as fit() leaves it)
                    model._initialize(given_parameters, kwargs)
                    model._setup_fitting_parameters(fitting)
                    batch.upload_member(slot_of[i], model.asignatures.X, model.adata.obsm["exposures"])
                    if model.weights_kl is not None or model.weights_lhalf is not None:
                        batch.set_weights(slot_of[i], model.weights_kl, model.weights_lhalf)
                    self._close_engine(model)  # (a sweep holds no per-member engine)
                    t_init += time.perf_counter() - ta
                else:
                    model.fit(self._member_adata(adata, r), given_parameters, kwargs, fitting, history=history)
                    model.compute_reconstruction_errors()
                    self._close_engine(model)
                    t_fallback += time.perf_counter() - ta
                    if F:
                        ta = time.perf_counter()
                        model.adata.obs["heldout_error"] = self._heldout_single(model, r)
                        t_heldout += time.perf_counter() - ta
                models.append(model)
            tb = time.perf_counter()
            steps = 0
            if batch is not None:
                n_iters, objectives, steps = self._batched_loop(batch, len(batch_ids), n_given)
                kl = batch.samplewise_kl()
                for i, j in slot_of.items():
                    model = models[i]
                    W, H = batch.download_member(j)
                    model.asignatures.X = W
                    model.adata.obsm["exposures"] = H
                    model.n_iterations_ = n_iters[j]
                    if history:
                        model.history["objective_function"] = objectives[j][1:]
                    model.adata.obs["reconstruction_error"] = kl[j]
            t_batched = time.perf_counter() - tb
            if F and batch is not None:
                # one launch over all batched members, each against the test half of its own split
                ta = time.perf_counter()
                held = batch.heldout_kl(list(slot_of.values()), [F + members[i][2] for i in slot_of], self.train_fraction)
                for row, i in zip(held, slot_of):
                    models[i].adata.obs["heldout_error"] = row
                t_heldout += time.perf_counter() - ta
            if self.stability:
                ta = time.perf_counter()
                self._run_stability(batch, slot_of, members, models, n_vars)
                t_stability = time.perf_counter() - ta
        finally:
            if batch is not None:
                batch.close()
        self.models_ = models
        self.batched_ = np.array([i in slot_of for i in range(len(members))], dtype=bool)
        cols = max(1, len(self.seeds or []))
        shape = (len(self.ns_signatures),) + ((len(self.lhalf_weights),) if self.lhalf_weights else ()) + (cols,) + ((R or F,) if R or F else ())
        self.reconstruction_errors_ = np.array([m.reconstruction_error for m in models]).reshape(shape)
        self.resample_of_ = np.array([-1 if F else r for _, _, r, _ in members], dtype=int)
        self.split_of_ = np.array([r if F else -1 for _, _, r, _ in members], dtype=int)
        self.lhalf_of_ = np.array([l for _, _, _, l in members], dtype=int)
        if F:
            self.heldout_errors_ = np.array([float(np.sum(np.asarray(m.adata.obs["heldout_error"]))) for m in models]).reshape(shape)
            self._summarise_heldout(self.reconstruction_errors_, self.heldout_errors_)
        self._fitted = True
        self.member_steps_ = steps
        self.timings_ = {"total_s": time.perf_counter() - t0, "init_s": t_init, "batched_s": t_batched, "fallback_s": t_fallback,
                         "resample_s": t_draw if R else 0.0}
        if self.stability:
            self.timings_["stability_s"] = t_stability
        if F:
            self.timings_["split_s"] = t_draw
            self.timings_["heldout_s"] = t_heldout
        return models

    def _next_stop(self, n_iteration: int) -> int:
        return SignatureNMF._next_stop(self, n_iteration)  # (reads conv_test_freq and max_iterations only)

    def _batched_loop(self, batch: BatchEngine, n_members: int, n_given: int):
        """SignatureNMF's fit loop (signature_nmf.py:369-405) for all members at once: the objective at iteration 0 and at
        every multiple of conv_test_freq, a member stops at its first test with ``rel_change < tol`` from min_iterations
        on, or at the cap.  Before min_iterations no test can stop anyone: steps and objectives are only queued and read
        in one go; from there on every test is read.  Returns the members' iteration counts, objective lists and the
        member-steps run."""
        freq = self.conv_test_freq
        objectives: list[list[float]] = [[] for _ in range(n_members)]
        n_iters = [0] * n_members
        pending: list[tuple[int, list[int]]] = []  # queued, unread rows of the objective array and their members
        next_row = 0

        def queue(members):
            nonlocal next_row
            if len(pending) == SLOTS:
                read()
            batch.objective_async(next_row, members)
            pending.append((next_row, list(members)))
            next_row = (next_row + 1) % SLOTS

        def read():
            while pending:
                first = pending[0][0]
                count = 1
                while count < len(pending) and pending[count][0] == first + count:
                    count += 1
                rows = batch.objective_read(first, count)
                for r in range(count):
                    for m in pending[r][1]:
                        objectives[m].append(float(rows[r][m]))
                del pending[:count]

        active = list(range(n_members))
        queue(active)
        n_iteration, steps = 0, 0
        while active:
            stop = self._next_stop(n_iteration)
            batch.kl_step(stop - n_iteration, active, [n_given] * len(active))
            steps += (stop - n_iteration) * len(active)
            n_iteration = stop
            last = n_iteration >= self.max_iterations
            if n_iteration % freq == 0:
                queue(active)
                if not last and n_iteration >= self.min_iterations:
                    read()
                    still = []
                    for m in active:
                        prev, cur = objectives[m][-2], objectives[m][-1]
                        if np.abs(prev - cur) / np.abs(prev) < self.tol:
                            n_iters[m] = n_iteration
                        else:
                            still.append(m)
                    active = still
            if last:
                for m in active:
                    n_iters[m] = n_iteration
                active = []
        read()
        return n_iters, objectives, steps
