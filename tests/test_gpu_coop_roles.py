"""The leftover round of the fused joint step in each of its forms (``csrc/salnmf_fused_kernel.h``: the pairing rule).

With ``tiles = 4 grid + L`` on a grid of ``grid`` workgroups of four waves the ``L`` leftover tiles run

* ``2 L <= grid``: as pairs -- workgroup ``b < L`` forms the tile's numerator share (role G), workgroup
  ``b + ceil(grid / 2)`` its U product and the H update (role U);
* ``L <= grid < 2 L``: as today's cooperative tile, both products in workgroup ``b``;
* ``L > grid``: as ordinary tiles, one wave each.

The shapes are the smallest that reach every branch, ``N = 16 (4 grid + L) - ragged`` with ``L`` at both ends of each form
and a partial last tile, for K = 50 (two remainder columns), 48 (none) and V = 83, K = 30 (masked feature columns).
Per case, after 1 and after 3 joint steps from a seeded start: W and H against the oracle entry by entry at the
tolerance of ``test_gpu_parity.py`` (``TOL``, there on the rel-L2 norm, here on every entry), two runs bit for bit, and
the objective folded into the first step (``kl_step_objective``) against the stand-alone one at that file's ``rtol``.
(With sample weights the engine does not fold -- there is no weighted instantiation with the objective -- so in the
weighted cases that assertion only holds the call's fall-back to the stand-alone value and its steps' bits.)

What no test here can show is the absence of a race between the two workgroups of a pair: role G reads the tile's old H
rows, role U stores its new ones, and a test passes whenever the timing happens to hold.  That is settled by construction
instead: the kernel pairs only in a pass whose output buffer is not its input (``p.Hout != p.H``), and the engine hands a
joint step of a pairing shape a buffer of its own and swaps (``salnmf.hip: kl_step_once``).  ``test_buffers_change_roles``
holds the host side of that: kept steps, the steps behind them and a rollback with the three H buffers in play.
"""

import numpy as np
import pytest
import torch

from oracle import klnmf_oracle as orc
from salamander_amd import Engine

pytestmark = pytest.mark.gpu

TOL = 1e-10        # test_gpu_parity.py: TOL
OBJ_RTOL = 1e-12   # test_gpu_parity.py: test_objective_folded_into_the_following_step


def cus():
    return int(torch.cuda.get_device_properties(0).multi_processor_count)


def leftover(which, grid):
    return {"one": 1, "half-1": grid // 2 - 1, "half": grid // 2, "half+1": grid // 2 + 1, "grid": grid, "grid+1": grid + 1}[which]


def form(L, grid):
    return "paired" if 2 * L <= grid else ("single" if L <= grid else "plain")


def run_case(V, K, which, ragged, weights=False, n_given=0):
    grid = cus()  # salnmf.hip, salnmf_create: min(compute units, ceil(tiles / 4)) -- every case has more than 4 tiles per unit
    L = leftover(which, grid)
    ntiles = 4 * grid + L
    N = 16 * ntiles - ragged
    want_form = {"one": "paired", "half-1": "paired", "half": "paired", "half+1": "single", "grid": "single", "grid+1": "plain"}[which]
    assert form(L, grid) == want_form
    X, W0, H0 = orc.synthetic_problem(V, N, K, seed=V + K + L + ragged)
    rng = np.random.default_rng(7)
    wk, wl = (rng.uniform(0.5, 2.0, N), rng.uniform(0.0, 0.3, N)) if weights else (None, None)

    engines = [Engine(N, V, K) for _ in range(3)]
    for e in engines:
        assert e.fused_grid() == min(grid, (ntiles + 3) // 4) == grid
        e.upload_X(X), e.upload_W(W0), e.upload_H(H0)
        e.set_weights(wk, wl)
    a, b, c = engines
    obj0 = a.objective()
    W, H = W0.T, H0.T
    done = 0
    for steps in (1, 3):
        for _ in range(steps - done):
            W, H = orc.update_WH(X.T, W, H, wk, wl, n_given)
        a.kl_step(steps - done, n_given), b.kl_step(steps - done, n_given)
        done = steps
        Wa, Ha = a.download_W(), a.download_H()
        errW = float(np.max(np.abs(Wa - W.T) / np.abs(W.T)))
        errH = float(np.max(np.abs(Ha - H.T) / np.abs(H.T)))
        print(f"[coop roles] V={V} K={K} L={L} ({want_form}) ragged={ragged} weights={weights} given={n_given} steps={steps}: "
              f"max entry error W {errW:.2e} H {errH:.2e}")
        assert np.allclose(Wa, W.T, rtol=TOL, atol=0) and np.allclose(Ha, H.T, rtol=TOL, atol=0)
        assert np.array_equal(Wa, b.download_W()) and np.array_equal(Ha, b.download_H())
    # the objective of the start, folded into the first of three steps: the value, and the steps' bits
    c.kl_step_objective(0, 3, n_given)
    folded = c.objective_read(0, 1)[0]
    print(f"[coop roles] objective folded {folded!r} stand-alone {obj0!r}")
    assert np.isclose(folded, obj0, rtol=OBJ_RTOL, atol=0)
    assert np.isclose(folded, orc.klnmf_objective(X.T, W0.T, H0.T, wk, wl), rtol=OBJ_RTOL, atol=0)
    assert np.array_equal(c.download_W(), Wa) and np.array_equal(c.download_H(), Ha)
    for e in engines:
        e.close()


@pytest.mark.parametrize("ragged", [0, 5])
@pytest.mark.parametrize("which", ["one", "half-1", "half", "half+1", "grid", "grid+1"])
@pytest.mark.parametrize("V,K", [(96, 50), (96, 48), (83, 30)])
def test_leftover_round_every_form(V, K, which, ragged):
    run_case(V, K, which, ragged)


@pytest.mark.parametrize("ragged", [0, 5])
@pytest.mark.parametrize("V,K", [(96, 50), (96, 48), (83, 30)])
def test_paired_form_with_sample_weights(V, K, ragged):
    """``weights_kl`` + ``weights_lhalf`` at L = grid / 2: role G scales its H operand, role U takes the l-half root."""
    run_case(V, K, "half", ragged, weights=True)


@pytest.mark.parametrize("ragged", [0, 5])
@pytest.mark.parametrize("V,K", [(96, 50), (96, 48), (83, 30)])
def test_paired_form_with_given_signatures(V, K, ragged):
    run_case(V, K, "half", ragged, n_given=2)


@pytest.mark.parametrize("which", ["half", "grid"])
def test_buffers_change_roles(which):
    """A step of a pairing shape writes the new H to a buffer of its own; a kept step writes the kept-state buffer.  Kept
    steps followed by plain ones equal plain steps bit for bit, a rollback restores the state the kept block started from,
    and the steps after it equal the plain ones again (L = grid: the in-place form, for comparison)."""
    V, K = 96, 50
    grid = cus()
    N = 16 * (4 * grid + leftover(which, grid)) - 5
    X, W0, H0 = orc.synthetic_problem(V, N, K, seed=11)
    a, b = Engine(N, V, K), Engine(N, V, K)
    for e in (a, b):
        e.upload_X(X), e.upload_W(W0), e.upload_H(H0)
        e.kl_step(2)
    W2, H2 = a.download_W(), a.download_H()
    assert np.array_equal(W2, b.download_W()) and np.array_equal(H2, b.download_H())
    a.kl_step(3)
    b.kl_step_keep(3)
    assert np.array_equal(a.download_W(), b.download_W()) and np.array_equal(a.download_H(), b.download_H())
    b.kl_rollback()
    assert np.array_equal(b.download_W(), W2) and np.array_equal(b.download_H(), H2)
    b.kl_step(3)
    assert np.array_equal(a.download_W(), b.download_W()) and np.array_equal(a.download_H(), b.download_H())
    W, H = W0.T, H0.T
    for _ in range(5):
        W, H = orc.update_WH(X.T, W, H)
    assert np.allclose(b.download_W(), W.T, rtol=TOL, atol=0) and np.allclose(b.download_H(), H.T, rtol=TOL, atol=0)
    a.close(), b.close()
