"""The weighted instantiation of the small-cohort body (``csrc/salnmf_small.hip``: ``small_kl_body<..., WTS = true>``),
through ``BatchEngine.set_weights`` against ``Engine.set_weights``.

A weighted engine takes the per-step path (``fused_kernel<..., WTS>`` + the W tail), which is the reference: W, H, the
queued objective and the per-sample divergences of a weighted batch member must equal the engine's bit for bit.  The shapes
follow the kernel's branches: 1, 7, 12, 16 and 19 tiles (every NG, a pad row, several tiles per wave), 64 tiles once;
K = 3, 7, 16 (contraction depths 1, 2, 4); one, two and seven steps (seven: the resident H and weights, the last-step stores).
Independent of the engine, one case per weight kind is held to ``oracle.update_WH`` within the tolerance
``tests/test_gpu_parity.py`` uses for its weighted steps."""
import numpy as np
import pytest

from oracle import klnmf_oracle as orc
from salamander_amd.batch import BatchEngine
from salamander_amd.engine import Engine

pytestmark = pytest.mark.gpu

TOL = 1e-10  # rel-L2 on W, H: tests/test_gpu_parity.py's TOL


def rel_l2(a, b):
    return float(np.linalg.norm(a - b) / np.linalg.norm(b))


def weights(kind, N, seed):
    rng = np.random.default_rng(1000 + seed)
    wkl, wlh = rng.uniform(0.5, 2.0, N), rng.uniform(0.0, 3.0, N)
    if kind == "kl":
        return wkl, None
    if kind == "lhalf":
        return None, wlh
    if kind == "both":
        return wkl, wlh
    if kind == "lhalf_zero":
        return None, np.zeros(N)
    if kind == "kl_with_zero":  # (without w_lhalf: the penalised form divides by w_kl^2, NaN in the reference too)
        wkl[N // 2] = 0.0
        return wkl, None
    raise ValueError(kind)


def problem(N, V, K, seed):
    X, W0, H0 = orc.synthetic_problem(V, N, K, seed=seed)
    return np.ascontiguousarray(X), np.ascontiguousarray(W0), np.ascontiguousarray(H0)


def engine_state(X, W0, H0, wkl, wlh, steps, n_given):
    N, V = X.shape
    e = Engine(N, V, W0.shape[0])
    try:
        e.upload_X(X), e.upload_W(W0), e.upload_H(H0)
        e.set_weights(wkl, wlh)
        e.kl_step(steps, n_given)
        return e.download_W(), e.download_H(), e.objective(), np.asarray(e.samplewise_kl())
    finally:
        e.close()


# a covering subset: every N and both V with some K, every K, both n_given, both step counts and every weight kind
CASES = [
    # N, V, K, n_given, steps, kind
    (13, 96, 3, 0, 1, "both"),
    (13, 83, 16, 1, 7, "lhalf"),
    (100, 96, 7, 0, 7, "kl"),
    (100, 83, 3, 1, 1, "lhalf_zero"),
    (180, 96, 16, 0, 7, "both"),
    (180, 83, 7, 1, 2, "kl_with_zero"),  # (w_kl alone reaches H through W: from the second step on)
    (250, 96, 3, 1, 7, "kl_with_zero"),
    (250, 83, 16, 0, 1, "lhalf"),
    (300, 96, 7, 0, 7, "kl"),
    (300, 83, 16, 1, 1, "both"),
    (300, 96, 3, 0, 7, "lhalf_zero"),
    (1024, 96, 16, 0, 2, "both"),
]


@pytest.mark.parametrize("N,V,K,n_given,steps,kind", CASES)
def test_weighted_member_equals_the_weighted_engine(N, V, K, n_given, steps, kind):
    X, W0, H0 = problem(N, V, K, seed=N + K)
    wkl, wlh = weights(kind, N, seed=N + K)
    W_ref, H_ref, obj_ref, skl_ref = engine_state(X, W0, H0, wkl, wlh, steps, n_given)
    b = BatchEngine(N, V, [K, K])
    try:
        b.upload_X(X)
        for m in range(2):
            b.upload_member(m, W0, H0)
        b.set_weights(0, wkl, wlh)  # member 1: the unweighted twin
        b.kl_step(steps, [0, 1], [n_given, n_given])
        b.objective_async(0, [0])
        W, H = b.download_member(0)
        _, H_plain = b.download_member(1)
        assert np.array_equal(W, W_ref)
        assert np.array_equal(H, H_ref)
        assert b.objective_read(0, 1)[0][0] == obj_ref
        assert np.array_equal(b.samplewise_kl()[0], skl_ref)
        assert not np.array_equal(H, H_plain)  # (a kernel that ignores the weights does not pass)
    finally:
        b.close()


def test_mixed_call_and_cleared_weights_leave_the_unweighted_bits():
    N, V, Ks, steps = 180, 96, [3, 7, 16, 5], 7
    probs = [problem(N, V, K, seed=K) for K in Ks]
    X = probs[0][0]
    wkl, wlh = weights("both", N, seed=1)

    def run(weighted):
        b = BatchEngine(N, V, Ks)
        try:
            b.upload_X(X)
            for m, (_, W0, H0) in enumerate(probs):
                b.upload_member(m, W0, H0)
            for m in weighted:
                b.set_weights(m, wkl, wlh)
            b.kl_step(steps, [0, 1, 2, 3], [0, 1, 0, 0])
            b.objective_async(0, [0, 1, 2, 3])
            return [b.download_member(m) for m in range(4)], b.objective_read(0, 1)[0].copy()
        finally:
            b.close()

    plain, plain_obj = run([])
    mixed, mixed_obj = run([1, 2])
    for m in (0, 3):  # the unweighted members of the mixed call: the bits of a batch that never saw weights
        assert np.array_equal(mixed[m][0], plain[m][0]) and np.array_equal(mixed[m][1], plain[m][1])
        assert mixed_obj[m] == plain_obj[m]
    for m in (1, 2):
        assert not np.array_equal(mixed[m][1], plain[m][1])
        _, W0, H0 = probs[m]
        W_ref, H_ref, obj_ref, _ = engine_state(X, W0, H0, wkl, wlh, steps, [0, 1, 0, 0][m])
        assert np.array_equal(mixed[m][0], W_ref) and np.array_equal(mixed[m][1], H_ref) and mixed_obj[m] == obj_ref

    # set_weights(m, None, None) returns a member to the unweighted bits
    b = BatchEngine(N, V, Ks)
    try:
        b.upload_X(X)
        for m, (_, W0, H0) in enumerate(probs):
            b.upload_member(m, W0, H0)
        b.set_weights(2, wkl, wlh)
        b.kl_step(1, [2], [0])
        b.set_weights(2, None, None)
        b.upload_member(2, probs[2][1], probs[2][2])
        b.kl_step(steps, [0, 1, 2, 3], [0, 1, 0, 0])
        for m in range(4):
            W, H = b.download_member(m)
            assert np.array_equal(W, plain[m][0]) and np.array_equal(H, plain[m][1])
    finally:
        b.close()


@pytest.mark.parametrize("kind", ["kl", "lhalf", "both", "lhalf_zero", "kl_with_zero"])
def test_weighted_member_against_the_oracle(kind):
    N, V, K, n_given, steps = 100, 96, 7, 1, 2
    X, W0, H0 = problem(N, V, K, seed=5)
    wkl, wlh = weights(kind, N, seed=5)
    W, H = W0.T, H0.T
    for _ in range(steps):
        W, H = orc.update_WH(X.T, W, H, wkl, wlh, n_given)
    b = BatchEngine(N, V, [K])
    try:
        b.upload_X(X)
        b.upload_member(0, W0, H0)
        b.set_weights(0, wkl, wlh)
        b.kl_step(steps, [0], [n_given])
        b.objective_async(0, [0])
        Wb, Hb = b.download_member(0)
        print(kind, rel_l2(Wb, W.T), rel_l2(Hb, H.T))
        assert rel_l2(Wb, W.T) < TOL and rel_l2(Hb, H.T) < TOL
        assert np.isclose(b.objective_read(0, 1)[0][0], orc.klnmf_objective(X.T, W, H, wkl, wlh), rtol=1e-12)
    finally:
        b.close()


def test_set_weights_refuses_bad_entries_before_copying():
    N, V, K = 20, 96, 3
    X, W0, H0 = problem(N, V, K, seed=2)
    b = BatchEngine(N, V, [K])
    try:
        b.upload_X(X)
        b.upload_member(0, W0, H0)
        for bad in (-1.0, np.nan, np.inf):
            w = np.ones(N)
            w[3] = bad
            with pytest.raises(RuntimeError):
                b.set_weights(0, w, None)
            with pytest.raises(RuntimeError):
                b.set_weights(0, None, w)
        with pytest.raises(RuntimeError):
            b.set_weights(1, np.ones(N), None)
        b.kl_step(1, [0], [0])  # still unweighted: nothing was copied
        W_ref, H_ref, _, _ = engine_state(X, W0, H0, None, None, 1, 0)
        W, H = b.download_member(0)
        assert np.array_equal(W, W_ref) and np.array_equal(H, H_ref)
    finally:
        b.close()
