"""``FakeResampleBatchEngine`` with count splits and held-out scoring -- TESTS ONLY.

The splits come from the NumPy replica (``_split_ref``): train split f is dataset f, test split f dataset F + f.  Held-out
scoring runs the oracle's per-sample divergence on the clipped test half with the scaled, clipped exposures.  ``planted``
replaces what the sweep reads back by chosen numbers: ``{"train": [...], "heldout": [...]}``, one value per member, returned
as that member's first per-sample entry (the others 0), so the sums are the planted values exactly."""

import numpy as np

import _split_ref as ref
from _fake_resample_batch_engine import FakeResampleBatchEngine
from oracle import klnmf_oracle as orc


class FakeSplitBatchEngine(FakeResampleBatchEngine):
    instances = []
    planted = None

    def __init__(self, n_samples, n_features, n_signatures, device=0):
        super().__init__(n_samples, n_features, n_signatures, device)
        FakeSplitBatchEngine.instances.append(self)
        self.split_calls = []    # (n_splits, train_fraction, seed)
        self.heldout_calls = []  # (members, datasets, train_fraction)

    def split(self, n_splits, train_fraction=0.5, seed=0):
        assert self.slots is None, "splits and resamples exclude each other"
        self.split_calls.append((n_splits, train_fraction, seed))
        train, test = ref.split_counts(self.raw_X, n_splits, train_fraction, seed)
        self.counts = np.concatenate([train, test])
        self.slots = self.counts.clip(orc.EPSILON)
        self.dataset = [-1] * self.M

    def _rows(self, values):
        out = np.zeros((len(values), self.N))
        out[:, 0] = values
        return out

    def samplewise_kl(self):
        if self.planted is not None:
            return self._rows(self.planted["train"])
        return super().samplewise_kl()

    def heldout_kl(self, members, datasets, train_fraction=0.5):
        self.heldout_calls.append((list(members), list(datasets), train_fraction))
        if self.planted is not None:
            return self._rows([self.planted["heldout"][m] for m in members])
        c = (1.0 - train_fraction) / train_fraction
        return np.stack([
            orc.samplewise_kl_divergence(self.slots[d].T, self.W[m].T, np.maximum(c * self.H[m], float(orc.EPSILON)).T)
            for m, d in zip(members, datasets)
        ])
