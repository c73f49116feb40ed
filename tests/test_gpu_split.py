"""The device's count splitting against its NumPy replica (``_split_ref``), entry by entry.

Everything in the contract is integer arithmetic, so ``sal.split_counts`` and ``BatchEngine.split`` must give the replica's
matrices exactly -- ``np.array_equal``, every entry of every case -- and the same bits on every call."""
import numpy as np
import pytest

import _resample_ref
import _split_ref as ref
import salamander_amd as sal
from salamander_amd.batch import BatchEngine

pytestmark = pytest.mark.gpu

EPSILON = 1.1920928955078125e-07
SEEDS = [0, 2**40 + 3]  # (the second has both key words non-zero)


def edge_rows(V, rng):
    """Seven rows of V cells: T = 0; T = 1 (an odd total: only the first half of a block is used); T = 2; T = 3; T = 513
    (more Philox blocks than lanes: the lanes stride); one cell of 5 000 mutations spanning many blocks; and a row whose
    only mass is in the last cell."""
    X = np.zeros((7, V))
    X[1, V // 2] = 1
    X[2, 0] = 2
    X[3, 0] += 1
    X[3, V // 3] += 2
    X[4] = rng.multinomial(513, np.full(V, 1.0 / V))
    X[5, V // 4] = 5000
    X[6, -1] = 9
    assert list(X.sum(axis=1)) == [0, 1, 2, 3, 513, 5000, 9] and (X[6, :-1] == 0).all()
    return X


def edge_matrix(N, V, rng):
    """N = 1: T = 513 spread over the cells plus 5 000 in the last one.  N = 5: the rows of T = 0, 1, 3, 513 and 5 000."""
    X = edge_rows(V, rng)
    if N == 1:
        X[4, -1] += 5000
        return X[4:5].copy()
    return X[[0, 1, 3, 4, 5]].copy()


def check(X, F, p, seed):
    N, V = X.shape
    want_train, want_test = ref.split_counts(X, F, p, seed)
    train, test = sal.split_counts(X, F, train_fraction=p, seed=seed)
    assert train.dtype == test.dtype == np.float64 and train.shape == test.shape == (F, N, V)
    assert np.array_equal(train, want_train) and np.array_equal(test, want_test)
    assert np.array_equal(train + test, np.broadcast_to(X, train.shape)) and (train[:, X == 0] == 0).all() and (test[:, X == 0] == 0).all()


@pytest.mark.parametrize("seed", SEEDS)
@pytest.mark.parametrize("p", [0.5, 0.8])
@pytest.mark.parametrize("F", [1, 3])
@pytest.mark.parametrize("N,V", [(1, 1), (5, 1), (1, 7), (5, 7), (1, 96), (5, 96), (1, 97), (5, 97), (1, 3072)])
def test_stand_alone_raw_layout(N, V, F, p, seed):
    check(edge_matrix(N, V, np.random.default_rng(V)), F, p, seed)


@pytest.mark.parametrize("seed", SEEDS)
@pytest.mark.parametrize("V", [7, 96, 3072])
def test_all_edge_rows_in_one_call(V, seed):
    check(edge_rows(V, np.random.default_rng(V)), 3, 0.8, seed)


@pytest.mark.parametrize("seed", SEEDS)
def test_split_f_does_not_depend_on_the_number_of_splits_and_a_call_repeats_its_bits(seed):
    X = edge_matrix(5, 96, np.random.default_rng(1))
    five = sal.split_counts(X, 5, train_fraction=0.5, seed=seed)
    two = sal.split_counts(X, 2, train_fraction=0.5, seed=seed)
    assert np.array_equal(two[0], five[0][:2]) and np.array_equal(two[1], five[1][:2])
    again = sal.split_counts(X, 5, train_fraction=0.5, seed=seed)
    assert np.array_equal(again[0], five[0]) and np.array_equal(again[1], five[1])
    assert not np.array_equal(five[0][0], five[0][1])


@pytest.mark.parametrize("V", [7, 96])
def test_batch_layout(V):
    """N = 17 (one pad tile row short of 32): all 2 F slots as the kernels read them, and as counts."""
    N, F, p, seed = 17, 3, 0.8, 2**40 + 3
    rng = np.random.default_rng(V)
    X = np.concatenate([edge_rows(V, rng), rng.poisson(rng.gamma(0.5, 20.0, size=(10, V))).astype(float)])
    want = np.concatenate(ref.split_counts(X, F, p, seed))  # train 0 .. F - 1 | test 0 .. F - 1
    alone = np.concatenate(sal.split_counts(X, F, train_fraction=p, seed=seed))
    assert np.array_equal(alone, want)
    b = BatchEngine(N, V, [2, 5])
    try:
        b.upload_X(X, clip=True)
        b.split(F, p, seed)
        Np = 16 * ((N + 15) // 16)
        for d in range(2 * F):
            assert np.array_equal(b.download_dataset(d), want[d]), d
            slot = b.download_dataset(d, raw=True)
            assert slot.shape == (Np, 96)
            assert np.array_equal(slot[:N, :V], np.maximum(want[d], EPSILON)), d
            assert (slot[N:] == 0).all() and (slot[:, V:] == 0).all(), d  # pad rows and columns exactly 0
        slot = b.download_dataset(-1, raw=True)  # the uploaded X is untouched by the draw
        assert np.array_equal(slot[:N, :V], np.maximum(X, EPSILON)) and (slot[N:] == 0).all() and (slot[:, V:] == 0).all()
        b.split(F, p, seed)
        assert np.array_equal(np.stack([b.download_dataset(d) for d in range(2 * F)]), want)
    finally:
        b.close()


def test_the_profile_entry_points_time_the_kernel_and_leave_the_draw_in_the_slots():
    """N = 17, V = 7: a pad row, pad columns and rows of more Philox blocks than lanes (T = 513 and T = 5 000).  The timed
    launches rewrite the slots with the same bits, so after a profile call the batch holds what the draw itself leaves."""
    N, V, seed = 17, 7, 2**40 + 3
    rng = np.random.default_rng(V)
    X = np.concatenate([edge_rows(V, rng), rng.poisson(rng.gamma(0.5, 20.0, size=(10, V))).astype(float)])
    b = BatchEngine(N, V, [2])
    try:
        b.upload_X(X, clip=True)
        ms = b.profile_split(3, 0.8, seed, n_calls=2)
        assert np.isfinite(ms) and ms > 0
        want = np.concatenate(ref.split_counts(X, 3, 0.8, seed))
        for d in range(6):
            assert np.array_equal(b.download_dataset(d), want[d]), d
            slot = b.download_dataset(d, raw=True)
            assert (slot[N:] == 0).all() and (slot[:, V:] == 0).all(), d  # pad rows and columns exactly 0
        b.upload_X(X, clip=True)
        ms = b.profile_resample(2, seed, n_calls=2)
        assert np.isfinite(ms) and ms > 0
        want = _resample_ref.resample_counts(X, 2, seed)
        for d in range(2):
            assert np.array_equal(b.download_dataset(d), want[d]), d
    finally:
        b.close()


def test_the_library_refuses_bad_arguments_before_any_launch():
    """The C entry points themselves (Python validates earlier): status 1 and a message through the usual channel."""
    from salamander_amd import _lib
    from salamander_amd.engine import _ptr

    lib = _lib.load()
    half = 2**63
    out = np.empty((1, 2, 3))
    good = np.ascontiguousarray([[1.0, 2, 3], [1, 5, 0]])
    for X, word in ((np.array([[1, 2, 3], [1, 0.5, 0]]), "row 1"), (np.array([[1, -2, 3], [1, 1, 0]]), "row 0"),
                    (np.array([[1, 2, 3], [2.0**31, 2.0**31, 0]]), "row 1")):
        X = np.ascontiguousarray(X, dtype=np.float64)
        assert lib.salnmf_split_counts(0, _ptr(X), 2, 3, 1, half, 0, _ptr(out), _ptr(out)) == 1
        assert word in _lib.last_error()
    assert lib.salnmf_split_counts(0, _ptr(good), 2, 3, 0, half, 0, _ptr(out), _ptr(out)) == 1 and "n_splits" in _lib.last_error()
    assert lib.salnmf_split_counts(0, _ptr(good), 2, 3, 1, 0, 0, _ptr(out), _ptr(out)) == 1 and "threshold" in _lib.last_error()
    assert lib.salnmf_split_counts(0, None, 2, 3, 1, half, 0, _ptr(out), _ptr(out)) == 1 and "null" in _lib.last_error()
    assert lib.salnmf_split_counts(0, _ptr(good), 2, 3, 1, half, 0, _ptr(out), None) == 1 and "null" in _lib.last_error()
    assert lib.salnmf_split_counts(0, _ptr(good), 2, 3073, 1, half, 0, _ptr(out), _ptr(out)) == 1 and "n_features" in _lib.last_error()
    b = BatchEngine(2, 3, [1, 2])
    try:
        with pytest.raises(RuntimeError, match="upload X first"):
            b.split(2)
        b.upload_X(np.array([[1, 2, 3], [1, 0.5, 0]]), clip=True)
        with pytest.raises(RuntimeError, match="row 1"):
            b.split(2)
        b.upload_X(good, clip=True)
        assert lib.salnmf_batch_split(b._h, 0, half, 0) == 1 and "n_splits" in _lib.last_error()
        assert lib.salnmf_batch_split(b._h, 2, 0, 0) == 1 and "threshold" in _lib.last_error()
        with pytest.raises(RuntimeError, match="out of range"):
            b.set_dataset(0, 0)  # (no split drawn yet)
        b.split(2)
        with pytest.raises(RuntimeError, match="out of range"):
            b.set_dataset(0, 4)
        b.set_dataset(0, 3)
        with pytest.raises(RuntimeError, match="exclude each other"):
            b.resample(2)
        with pytest.raises(RuntimeError, match="out of range"):
            b.heldout_kl([0], [4])
        with pytest.raises(RuntimeError, match="out of range"):
            b.heldout_kl([2], [0])
        with pytest.raises(RuntimeError, match="twice"):
            b.heldout_kl([1, 1], [2, 3])
        out2 = np.empty((1, 2))
        m = np.zeros(1, dtype=np.int32)
        iptr = m.ctypes.data_as(_lib._I)
        assert lib.salnmf_batch_heldout_kl(b._h, 1, iptr, None, 1.0, _ptr(out2)) == 1 and "null" in _lib.last_error()
        assert lib.salnmf_batch_heldout_kl(b._h, 1, iptr, iptr, 1.0, None) == 1 and "null" in _lib.last_error()
        assert lib.salnmf_batch_heldout_kl(b._h, 1, iptr, iptr, 0.0, _ptr(out2)) == 1 and "scale" in _lib.last_error()
        b.upload_X(good, clip=True)  # drops the split: resamples are allowed again, and then a split is refused
        b.resample(2)
        with pytest.raises(RuntimeError, match="exclude each other"):
            b.split(2)
    finally:
        b.close()
