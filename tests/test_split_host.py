"""Count splitting on the CPU: the NumPy replica of the device's thinning kernel against the properties of its contract and
against the binomial law, and the argument validation of ``sal.split_counts`` and ``KLNMFSweep``.

The device itself is compared with the replica entry by entry in tests/test_gpu_split.py."""

from fractions import Fraction

import numpy as np
import pytest

import _resample_ref as rref
import _split_ref as ref
import salamander_amd as sal


@pytest.fixture(scope="module")
def counts():
    rng = np.random.default_rng(5)
    X = rng.poisson(rng.gamma(0.4, 30.0, size=(9, 23))).astype(float)
    X[3] = 0        # a sample without mutations
    X[:, 11] = 0    # a feature nobody has
    return X


def test_halves_add_up_zero_cells_stay_zero_and_split_f_does_not_depend_on_the_number_of_splits(counts):
    train, test = ref.split_counts(counts, 5, 0.5, seed=11)
    assert train.shape == test.shape == (5, 9, 23)
    assert np.array_equal(train, np.floor(train)) and (train >= 0).all() and (test >= 0).all()
    assert np.array_equal(train + test, np.broadcast_to(counts, train.shape))
    assert (train[:, counts == 0] == 0).all() and (test[:, counts == 0] == 0).all()
    two = ref.split_counts(counts, 2, 0.5, seed=11)
    assert np.array_equal(two[0], train[:2]) and np.array_equal(two[1], test[:2])
    assert not np.array_equal(train[0], train[1])
    assert not np.array_equal(ref.split_counts(counts, 1, 0.5, seed=12)[0][0], train[0])
    assert not np.array_equal(ref.split_counts(counts, 1, 0.5, seed=11 + 2**32)[0][0], train[0])  # the key's high word counts
    # a larger fraction moves mutations to train only: the draws are the same, the threshold is higher
    more = ref.split_counts(counts, 1, 0.8, seed=11)[0][0]
    assert (more >= train[0]).all() and more.sum() > train[0].sum()


def test_the_stream_is_not_the_resamplers():
    """Counter word 1 is 0x53504C54 here and 0 in the resampler: the same (seed, n, r = f) gives other blocks."""
    seed, n, f, T = 7, 3, 2, 64
    q = np.arange(T // 2, dtype=np.uint64)
    o = rref.philox4x32_10(q, np.zeros_like(q), np.full_like(q, n), np.full_like(q, f), seed & 0xFFFFFFFF, seed >> 32)
    theirs = np.stack([o[0] | (o[1] << rref.S32), o[2] | (o[3] << rref.S32)], axis=1).reshape(-1)
    mine = ref.draws(T, n, f, seed)
    assert mine.dtype == np.uint64 and len(mine) == T and not np.isin(mine, theirs).any()
    assert np.array_equal(ref.draws(T - 1, n, f, seed), mine[:-1])  # an odd total uses the first half of the last block


@pytest.mark.parametrize("p", [0.5, 0.8, 0.1, 2.0**-40])
def test_the_threshold_is_the_exact_floor(p):
    from salamander_amd.split import train_threshold

    want = (Fraction(p) * 2**64).__floor__()
    assert ref.threshold(p) == want == train_threshold(p) and 1 <= want <= 2**64 - 1


def test_train_counts_follow_the_binomial_law():
    """One row of 8 cells with counts 0 .. 4 000, F = 200 splits at p = 0.3, seed 2024.  Per cell the mean of the train
    counts lies within 4 standard errors of c p (two-sided 6.3e-5 per cell).  Pearson's statistic
    sum_{f, c > 0} (train - c p)^2 / (c p (1 - p)) has 200 x 7 = 1 400 terms of mean 1 and variance 2 + (1 - 6 p q) / (c p q)
    <= 2.03 (c >= 40): a chi-square of 1 400 degrees of freedom to that accuracy, whose 99.9 % point by Wilson and Hilferty's
    cube-root formula is 1 569.2.  The replica gives 1 415.0.  A threshold off by a factor, or a cell search off by
    one, moves it by thousands."""
    row = np.array([[0, 40, 100, 250, 500, 1000, 2000, 4000]], dtype=float)
    F, p, q = 200, 0.3, 0.7
    train, test = ref.split_counts(row, F, p, seed=2024)
    c = row[0]
    assert (train[:, 0, 0] == 0).all() and np.array_equal(train + test, np.broadcast_to(row, train.shape))
    nz = c > 0
    mean = train[:, 0, nz].mean(axis=0)
    assert (np.abs(mean - c[nz] * p) < 4.0 * np.sqrt(c[nz] * p * q / F)).all(), mean - c[nz] * p
    chi2 = float((((train[:, 0, nz] - c[nz] * p) ** 2) / (c[nz] * p * q)).sum())
    dof = F * int(nz.sum())
    z999 = 3.090232306167813
    cut = dof * (1.0 - 2.0 / (9.0 * dof) + z999 * np.sqrt(2.0 / (9.0 * dof))) ** 3
    print(f"chi2 {chi2:.1f}, dof {dof}, 99.9 % point {cut:.1f}")
    assert dof == 1400 and abs(cut - 1569.2) < 0.1
    assert chi2 < cut, chi2


def test_split_counts_validates_on_the_host():
    X = np.ones((3, 4))
    for bad, match in ((X * 0.5, "row 0"), (-X, "row 0"), (np.ones(4), "matrix")):
        with pytest.raises(ValueError, match=match):
            sal.split_counts(bad, 2)
    for bad in (0, -1, 1.5, True, 40000):
        with pytest.raises(ValueError, match="n_splits"):
            sal.split_counts(X, bad)
    for bad in (0.0, 1.0, -0.2, 1.5, 1, "half", None, float("nan"), 1e-30):
        with pytest.raises(ValueError, match="train_fraction"):
            sal.split_counts(X, 1, train_fraction=bad)
    with pytest.raises(ValueError, match="seed"):
        sal.split_counts(X, 1, seed=-3)
    with pytest.raises(ValueError, match="columns"):
        sal.split_counts(np.ones((2, 3073)), 1)


def test_the_sweep_validates_in_its_constructor():
    for bad in (-1, 1.5, True, 40000):
        with pytest.raises(ValueError, match="n_splits"):
            sal.models.KLNMFSweep([2], n_splits=bad)
    for bad in (0.0, 1.0, 2, "x"):
        with pytest.raises(ValueError, match="train_fraction"):
            sal.models.KLNMFSweep([2], n_splits=2, train_fraction=bad)
    for bad in (-1, 2**64, 0.5):
        with pytest.raises(ValueError, match="seed"):
            sal.models.KLNMFSweep([2], n_splits=2, split_seed=bad)
    with pytest.raises(ValueError, match="exclude each other"):
        sal.models.KLNMFSweep([2], n_splits=2, n_resamples=2)
    s = sal.models.KLNMFSweep([2], n_splits=3, train_fraction=0.8, split_seed=9)
    assert (s.n_splits, s.train_fraction, s.split_seed) == (3, 0.8, 9)
    assert sal.models.KLNMFSweep([2]).n_splits == 0
