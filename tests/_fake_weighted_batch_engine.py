"""``FakeBatchEngine`` (through its split-capable subclass) with per-member weights -- TESTS ONLY.

``set_weights`` records the vectors; the steps and objectives of a member run the oracle's weighted ``update_WH`` /
``klnmf_objective`` on the member's own dataset, exactly what ``_fake_engine.FakeEngine`` runs for a single weighted fit.
The per-sample and held-out divergences stay unweighted, as on the device."""

import numpy as np

from _fake_split_batch_engine import FakeSplitBatchEngine
from oracle import klnmf_oracle as orc


class FakeWeightedBatchEngine(FakeSplitBatchEngine):
    instances = []

    def __init__(self, n_samples, n_features, n_signatures, device=0):
        super().__init__(n_samples, n_features, n_signatures, device)
        FakeWeightedBatchEngine.instances.append(self)
        self.wkl = [None] * self.M
        self.wlh = [None] * self.M
        self.weight_calls = []  # members, in call order

    def set_weights(self, member, weights_kl=None, weights_lhalf=None):
        for w in (weights_kl, weights_lhalf):
            assert w is None or (np.shape(w) == (self.N,) and np.all(np.isfinite(w)) and np.all(np.asarray(w) >= 0))
        self.weight_calls.append(member)
        self.wkl[member] = None if weights_kl is None else np.array(weights_kl, dtype=float)
        self.wlh[member] = None if weights_lhalf is None else np.array(weights_lhalf, dtype=float)

    def kl_step(self, n_steps, members, n_given):
        self.step_calls.append((n_steps, list(members)))
        for m, g in zip(members, n_given):
            assert 0 <= g < self.Ks[m]
            for _ in range(n_steps):
                W, H = orc.update_WH(self._X(m).T, self.W[m].T, self.H[m].T, self.wkl[m], self.wlh[m], g)
                self.W[m], self.H[m] = W.T.copy(), H.T.copy()

    def objective_async(self, slot, members):
        self.queued.append((slot, list(members)))
        for m in members:
            self.rows[slot, m] = orc.klnmf_objective(self._X(m).T, self.W[m].T, self.H[m].T, self.wkl[m], self.wlh[m])
