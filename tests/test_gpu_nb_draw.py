"""``sal.draw_nb_counts`` on the device against the host replica (tests/_nbdraw_ref.py): every comparison is
``np.array_equal``."""

import numpy as np
import pytest

import _nbdraw_ref as ref
import salamander_amd as sal

pytestmark = pytest.mark.gpu

EPS = ref.EPSILON
N, B = 40, 3
ALPHAS = np.array([0.05, 0.5, 1.0, 20.0, 1e4, 1e6])
MEANS = np.array([0.0, 0.5, 9.9, 10.1, 255.0, 2000.0, 100000.0])  # the two Poisson paths and their seam at 10
SEED = 12345678901234567


def draw_case(K, V, seed):
    """Exposures with entries at exactly EPSILON and at 0, a signature row with zeros, the dispersions in turn (6 values) and the
    row means in turn (7 values): every mean meets every dispersion class within 40 rows' reach of 42."""
    rng = np.random.default_rng(seed)
    W = rng.dirichlet(np.full(V, 0.3), size=K)
    W[K // 2, rng.permutation(V)[: max(2, V // 3)]] = 0.0
    W = W / W.sum(axis=1, keepdims=True)
    H = rng.uniform(0.01, 1.0, size=(N, K))
    if K > 1:
        H[rng.random((N, K)) < 0.15] = EPS
        H[rng.random((N, K)) < 0.05] = 0.0
        H[:, 0] = np.maximum(H[:, 0], 0.01)
    means = MEANS[np.arange(N) % MEANS.size]
    H = H / H.sum(axis=1, keepdims=True) * means[:, None]
    if K > 1:
        H[9, 1] = EPS  # (after the scaling too)
    return H, W, ALPHAS[np.arange(N) % ALPHAS.size]


@pytest.mark.parametrize("K,V", [(1, 7), (3, 7), (17, 96), (96, 96)])
def test_draws_equal_the_replica(K, V):
    H, W, alpha = draw_case(K, V, seed=100 * K + V)
    got = sal.draw_nb_counts(H, W, alpha, B, seed=SEED)
    want, failed = ref.draw_nb_counts(H, W, alpha, B, seed=SEED)
    assert failed == 0 and got.shape == (B, N, V) and got.dtype == np.float64
    assert np.array_equal(got, want)
    assert not got[:, H.sum(axis=1) == 0].any()
    assert not got[:, :, ((H @ W) == 0).all(axis=0)].any()  # channels of mean 0 stay 0
    assert len(set(got[:, 6].sum(axis=1))) > 1  # the draw is unconditional: the totals of a row differ between draws


def test_draw_b_does_not_depend_on_the_number_of_draws_nor_on_the_other_rows():
    H, W, alpha = draw_case(17, 96, seed=5)
    d8 = sal.draw_nb_counts(H, W, alpha, 8, seed=3)
    assert np.array_equal(sal.draw_nb_counts(H, W, alpha, 4, seed=3), d8[:4])
    assert not np.array_equal(d8[0], d8[1]) and not np.array_equal(sal.draw_nb_counts(H, W, alpha, 1, seed=4)[0], d8[0])
    # the row index is a counter word: a subset or a permutation of the rows is another set of draws, the replica's at those indices
    subset = np.array([5, 6, 12, 13, 20, 39])
    got = sal.draw_nb_counts(H[subset], W, alpha[subset], 2, seed=3)
    assert np.array_equal(got, ref.draw_nb_counts(H[subset], W, alpha[subset], 2, seed=3)[0])
    # ... and row i of a call depends on nothing but its own exposures, dispersion and index: rows moved to the index they had
    perm = np.random.default_rng(0).permutation(N)
    moved_H, moved_alpha = H.copy(), alpha.copy()
    keep = perm[:20]
    others = np.setdiff1d(np.arange(N), keep)
    moved_H[others] = H[others][::-1] * 0.5
    moved_alpha[others] = alpha[others][::-1]
    assert np.array_equal(sal.draw_nb_counts(moved_H, W, moved_alpha, 4, seed=3)[:, keep], d8[:4][:, keep])
