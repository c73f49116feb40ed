"""``FakeResampleBatchEngine`` with ``stability`` -- TESTS ONLY.

The matching runs the NumPy replica (``_stability_ref``) on the members' signatures as the oracle left them; every call is
recorded with its groups, errors and round cap."""

import numpy as np

import _stability_ref as ref
from _fake_resample_batch_engine import FakeResampleBatchEngine
from salamander_amd.stability import StabilityResult


class FakeStabilityBatchEngine(FakeResampleBatchEngine):
    instances = []

    def __init__(self, n_samples, n_features, n_signatures, device=0):
        super().__init__(n_samples, n_features, n_signatures, device)
        FakeStabilityBatchEngine.instances.append(self)
        self.stability_calls = []  # (groups, errors, max_rounds)

    def stability(self, groups, errors=None, max_rounds=20):
        assert not self.closed, "the sweep must ask before it closes the batch"
        self.stability_calls.append(([list(g) for g in groups], None if errors is None else [list(e) for e in errors], max_rounds))
        out = []
        for g, members in enumerate(groups):
            assert len({self.Ks[m] for m in members}) == 1 and len(members) >= 2
            r = ref.stability(np.stack([self.W[m] for m in members]), None if errors is None else errors[g], max_rounds, margins=False)
            out.append(StabilityResult(r.assignments, r.n_rounds, r.converged, r.consensus, r.a, r.b, r.silhouette, r.cluster_stability,
                                       r.stability_mean, r.stability_min))
        return out
