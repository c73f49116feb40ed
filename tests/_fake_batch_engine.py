"""An oracle-backed stand-in for ``salamander_amd.batch.BatchEngine`` -- TESTS ONLY.

Runs each member through the same oracle functions as ``_fake_engine.FakeEngine``, so a sweep on this fake and single
fits on that one must agree bit for bit.  Records every step call and every read of the objective array."""

import numpy as np

from oracle import klnmf_oracle as orc


class FakeBatchEngine:
    instances = []

    def __init__(self, n_samples, n_features, n_signatures, device=0):
        self.N, self.V, self.device = n_samples, n_features, device
        self.Ks = [int(k) for k in n_signatures]
        self.M = len(self.Ks)
        self.W = [None] * self.M
        self.H = [None] * self.M
        self.rows = np.full((256, self.M), np.nan)
        self.step_calls = []  # (n_steps, members)
        self.reads = []       # (first, count)
        self.queued = []      # (slot, members)
        self.closed = False
        FakeBatchEngine.instances.append(self)

    def close(self):
        self.closed = True

    def upload_X(self, X, clip=False):
        self.X = np.array(X, dtype=float)
        if clip:
            self.X = self.X.clip(orc.EPSILON)

    def upload_member(self, member, W, H):
        assert np.shape(W) == (self.Ks[member], self.V) and np.shape(H) == (self.N, self.Ks[member])
        self.W[member] = np.array(W, dtype=float)
        self.H[member] = np.array(H, dtype=float)

    def download_member(self, member):
        return self.W[member].copy(), self.H[member].copy()

    def kl_step(self, n_steps, members, n_given):
        self.step_calls.append((n_steps, list(members)))
        for m, g in zip(members, n_given):
            assert 0 <= g < self.Ks[m]
            for _ in range(n_steps):
                W, H = orc.update_WH(self.X.T, self.W[m].T, self.H[m].T, None, None, g)
                self.W[m], self.H[m] = W.T.copy(), H.T.copy()

    def objective_async(self, slot, members):
        self.queued.append((slot, list(members)))
        for m in members:
            self.rows[slot, m] = orc.klnmf_objective(self.X.T, self.W[m].T, self.H[m].T, None, None)

    def objective_read(self, first, count):
        self.reads.append((first, count))
        return self.rows[first : first + count].copy()

    def samplewise_kl(self):
        return np.stack([orc.samplewise_kl_divergence(self.X.T, self.W[m].T, self.H[m].T) for m in range(self.M)])
