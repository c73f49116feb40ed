"""The device's bootstrap resampler against its NumPy replica (``_resample_ref``), entry by entry.

Everything in the contract is integer arithmetic, so ``sal.resample_counts`` and ``BatchEngine.resample`` must give the
replica's matrices exactly -- ``np.array_equal``, every entry of every case -- and the same bits on every call."""
import os

import numpy as np
import pytest

import _resample_ref as ref
import salamander_amd as sal
from conftest import GOLDEN, read_counts
from salamander_amd.batch import BatchEngine

pytestmark = pytest.mark.gpu

EPSILON = 1.1920928955078125e-07
SEEDS = [2024, 2**32 + 12345]  # (the second reaches the key's high word)


@pytest.fixture(scope="module")
def pcawg():
    return read_counts(os.path.join(GOLDEN, "pcawg_breast_sbs.csv")).T.values.astype(float)


def edge_rows(V, rng):
    """A zero row, a row with one non-zero cell, rows of an odd and an even total, and one of about 3e6 mutations (every
    lane of the workgroup passes over the Philox blocks many times)."""
    X = np.zeros((5, V))
    X[1, V // 3] = 1234
    X[2, : min(V, 7)] = [3, 0, 1, 4, 0, 2, 5][: min(V, 7)]
    X[2, 0] += 1 - X[2].sum() % 2  # odd total
    X[3, -5:] = [2, 0, 6, 1, 1]    # even total
    X[4] = rng.multinomial(3_000_001, rng.dirichlet(np.full(V, 0.3)))
    assert X[0].sum() == 0 and X[2].sum() % 2 == 1 and X[3].sum() % 2 == 0
    return X


def check_batch(X, R, seed, want):
    """BatchEngine.resample: the datasets as counts, and the slots as the kernels read them."""
    N, V = X.shape
    b = BatchEngine(N, V, [2, 5])
    try:
        b.upload_X(X, clip=True)
        b.resample(R, seed)
        Np = 16 * ((N + 15) // 16)
        for r in range(R):
            assert np.array_equal(b.download_dataset(r), want[r]), (seed, r)
            slot = b.download_dataset(r, raw=True)
            assert slot.shape == (Np, 96)
            assert np.array_equal(slot[:N, :V], np.maximum(want[r], EPSILON)), (seed, r)
            assert (slot[N:] == 0).all() and (slot[:, V:] == 0).all(), (seed, r)  # pad rows and columns exactly 0
        # the uploaded X is dataset -1, untouched by the draw, in the same layout
        slot = b.download_dataset(-1, raw=True)
        assert np.array_equal(slot[:N, :V], np.maximum(X, EPSILON)) and (slot[N:] == 0).all() and (slot[:, V:] == 0).all()
        again = b.download_dataset(0)
        b.resample(R, seed)
        assert np.array_equal(b.download_dataset(0), again)
    finally:
        b.close()


@pytest.mark.parametrize("seed", SEEDS)
def test_pcawg(pcawg, seed):
    R = 4
    want = ref.resample_counts(pcawg, R, seed)
    got = sal.resample_counts(pcawg, R, seed=seed)
    assert got.dtype == np.float64 and got.shape == (R, 192, 96)
    assert np.array_equal(got, want)
    assert np.array_equal(sal.resample_counts(pcawg, R, seed=seed), got)      # the same call twice: the same bits
    assert np.array_equal(sal.resample_counts(pcawg, 2, seed=seed), got[:2])  # resample r does not depend on R
    check_batch(pcawg, R, seed, want)


@pytest.mark.parametrize("seed", SEEDS)
def test_wide_synthetic_catalogue(seed):
    """N = 37 (not a multiple of 16), V = 1536: the prefix sums run over several entries per lane."""
    rng = np.random.default_rng(3)
    totals = rng.integers(50, 20000, size=37)
    X = np.stack([rng.multinomial(t, rng.dirichlet(np.full(1536, 0.05))) for t in totals]).astype(float)
    X = np.concatenate([X, edge_rows(1536, rng)])
    want = ref.resample_counts(X, 3, seed)
    got = sal.resample_counts(X, 3, seed=seed)
    assert np.array_equal(got, want)
    assert np.array_equal(sal.resample_counts(X, 3, seed=seed), got)
    assert np.array_equal(got.sum(axis=2), np.broadcast_to(X.sum(axis=1), (3, len(X)))) and (got[:, X == 0] == 0).all()


@pytest.mark.parametrize("seed", SEEDS)
@pytest.mark.parametrize("V", [96, 83])
def test_edge_rows_in_a_batch(pcawg, seed, V):
    """The edge rows after 32 PCAWG rows: N = 37, through both entry points."""
    rng = np.random.default_rng(V)
    X = np.concatenate([pcawg[:32, :V], edge_rows(V, rng)])
    want = ref.resample_counts(X, 2, seed)
    assert np.array_equal(sal.resample_counts(X, 2, seed=seed), want)
    check_batch(X, 2, seed, want)


def test_the_library_refuses_bad_counts_before_any_launch():
    """The C entry points themselves (Python validates earlier): status and message through the usual channel."""
    from salamander_amd import _lib
    from salamander_amd.engine import _ptr

    lib = _lib.load()
    out = np.empty((1, 2, 3))
    for X, word in ((np.array([[1, 2, 3], [1, 0.5, 0]]), "row 1"), (np.array([[1, -2, 3], [1, 1, 0]]), "row 0"),
                    (np.array([[1, 2, 3], [2.0**31, 2.0**31, 0]]), "row 1")):
        X = np.ascontiguousarray(X, dtype=np.float64)
        assert lib.salnmf_resample_counts(0, _ptr(X), 2, 3, 1, 0, _ptr(out)) != 0
        assert word in _lib.last_error()
    b = BatchEngine(2, 3, [1])
    try:
        with pytest.raises(RuntimeError, match="upload X first"):
            b.resample(2)
        b.upload_X(np.array([[1, 2, 3], [1, 0.5, 0]]), clip=True)
        with pytest.raises(RuntimeError, match="row 1"):
            b.resample(2)
        b.upload_X(np.array([[1.0, 2, 3], [1, 5, 0]]), clip=True)
        b.resample(2)
        with pytest.raises(RuntimeError, match="out of range"):
            b.set_dataset(0, 2)
        b.set_dataset(0, 1)
    finally:
        b.close()
