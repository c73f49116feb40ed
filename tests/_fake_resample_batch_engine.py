"""``FakeBatchEngine`` with bootstrap resamples -- TESTS ONLY.

The resamples come from the NumPy replica (``_resample_ref``), every member runs the oracle on its own dataset, and the
calls a sweep makes around them are recorded."""

import numpy as np

import _resample_ref as ref
from _fake_batch_engine import FakeBatchEngine
from oracle import klnmf_oracle as orc


class FakeResampleBatchEngine(FakeBatchEngine):
    instances = []  # (its own list: the parent class keeps the parent's)

    def __init__(self, n_samples, n_features, n_signatures, device=0):
        super().__init__(n_samples, n_features, n_signatures, device)
        FakeResampleBatchEngine.instances.append(self)
        self.dataset = [-1] * self.M
        self.slots = None
        self.resample_calls = []  # (n_resamples, seed)

    def upload_X(self, X, clip=False):
        self.raw_X = np.array(X, dtype=float)
        super().upload_X(X, clip)

    def resample(self, n_resamples, seed=0):
        self.resample_calls.append((n_resamples, seed))
        self.counts = ref.resample_counts(self.raw_X, n_resamples, seed)
        self.slots = self.counts.clip(orc.EPSILON)
        self.dataset = [-1] * self.M

    def set_dataset(self, member, dataset):
        assert -1 <= dataset < len(self.slots)
        self.dataset[member] = dataset

    def download_dataset(self, dataset, raw=False):
        assert not raw
        return self.X.copy() if dataset < 0 else self.counts[dataset].copy()

    def _X(self, m):
        return self.X if self.dataset[m] < 0 else self.slots[self.dataset[m]]

    def kl_step(self, n_steps, members, n_given):
        self.step_calls.append((n_steps, list(members)))
        for m, g in zip(members, n_given):
            assert 0 <= g < self.Ks[m]
            for _ in range(n_steps):
                W, H = orc.update_WH(self._X(m).T, self.W[m].T, self.H[m].T, None, None, g)
                self.W[m], self.H[m] = W.T.copy(), H.T.copy()

    def objective_async(self, slot, members):
        self.queued.append((slot, list(members)))
        for m in members:
            self.rows[slot, m] = orc.klnmf_objective(self._X(m).T, self.W[m].T, self.H[m].T, None, None)

    def samplewise_kl(self):
        return np.stack([orc.samplewise_kl_divergence(self._X(m).T, self.W[m].T, self.H[m].T) for m in range(self.M)])
