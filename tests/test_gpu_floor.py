"""The EPSILON clip floor on the device, entry by entry (``tests/_floor.py: assert_entrywise``).

Every update of the reference ends in ``clip(EPSILON)``.  On real (sparse) catalogues a large share of W and H sits at
that floor, but an entry of 1.2e-7 next to exposures of 1e3 weighs nothing in a rel-L2 norm: a kernel that left out a
clip, or wrote 0 instead of EPSILON, would pass the parity tests of ``test_gpu_parity.py``.  Here every case starts from a
state of the oracle on a sparse catalogue (``oracle.klnmf_oracle.floor_state``) with at least a quarter of H and of W at
the floor -- asserted, so that a change to the generator cannot make a case vacuous -- runs the device one step (and a
short run) and checks each entry: its relative error, that it is exactly EPSILON wherever the oracle's value before the
clip lies below the floor, and the NaN / inf pattern.  The oracle is pinned to the reference on such states by
``test_oracle_floor.py``.

Tolerances were measured on an MI355X; each constant notes the largest error seen over all cases that use it.
"""

import os
import sys

import numpy as np
import pytest

from _floor import EPS, assert_entrywise, floor_share, lhalf_allowance
from conftest import GOLDEN, ROOT
from oracle import klnmf_oracle as orc
from salamander_amd import Engine, _lib

pytestmark = pytest.mark.gpu

# entry-wise relative tolerances (max |dev - ref| / ref over every entry), each about 4-10x the largest error measured on
# an MI355X over all cases that use it (the kernels are deterministic: the same inputs give the same bits)
RT_STEP = 1e-13   # one fp64 step: 1.13e-14 (blocks1536x10, H)
RT_RUN = 1e-12    # five fp64 steps: 2.84e-13 (lhalf50, W)
RT_TRAJ = 5e-13   # fifty fp64 steps: 8.75e-14 (H)
RT_MV_W = 3e-8    # one MvNMF step, W: 5.04e-9 (mv288x10g2; the closed-form root of the volume majoriser cancels)
RT_MV_H = 3e-11   # one MvNMF step, H: 3.69e-12 (mv288x10g2)
RT_F32 = 5e-6     # the fp32 fast mode, one step: 9.92e-7 (f32/17000x8, H)
SKL_ABS = 1e-14   # per-sample KL, absolute error / (sum X + sum WH) of the sample: 1.18e-15 (skl288x12)
LHALF_C = 8.0     # roundings allowed in the l-half root's cancellation (tests/_floor.py: lhalf_allowance)


def _report(tag, worst):
    print(f"FLOORMAX {tag} {worst:.3e}")


def check(tag, dev, ref, rtol, pre=None, allowance=None, margin=1e-6):
    _report(tag, assert_entrywise(dev, ref, rtol, pre=pre, allowance=allowance, margin=margin, what=tag))


def active_for(K):
    """Active signatures per sample: up to four, fewer at small K so that a quarter of H can reach the floor."""
    return (1, max(1, min(4, K // 4)))


def state(V, N, K, seed, steps=40, wkl=None, wlh=None, n_given=0, check_h=True, check_w=True):
    X, W, H = orc.floor_state(V, N, K, seed, steps=steps, weights_kl=wkl, weights_lhalf=wlh, n_given=n_given, active=active_for(K))
    if check_h:
        assert floor_share(H) >= 0.25, f"input H: only {floor_share(H):.2f} at the floor"
    if check_w:
        assert floor_share(W) >= 0.25, f"input W: only {floor_share(W):.2f} at the floor"
    return X, W, H


def engine(X, W, H, wkl=None, wlh=None, small_tiles=0):
    N, V = X.shape
    e = Engine(N, V, W.shape[0])
    e.set_small_cohort_tiles(small_tiles)
    e.upload_X(X), e.upload_W(W), e.upload_H(H)
    e.set_weights(wkl, wlh)
    return e


def oracle_step(X, W, H, wkl=None, wlh=None, g=0):
    """One joint step of the oracle in sample-major layout: ``(W, H, W_pre, H_pre, H_allowance)``."""
    Wn, Hn = orc.update_WH(X.T, W.T, H.T, wkl, wlh, g)
    Wp, Hp, t, disc = orc.update_WH_preclip(X.T, W.T, H.T, wkl, wlh, g)
    allow = None if t is None else lhalf_allowance(t, disc, wkl, LHALF_C).T
    return Wn.T, Hn.T, Wp.T, Hp.T, allow


def step_and_run(tag, X, W, H, wkl=None, wlh=None, g=0, run=5, small_tiles=0, e=None):
    """One device step and then ``run - 1`` more, each compared with the oracle entry by entry."""
    K = W.shape[0]
    e = e or engine(X, W, H, wkl, wlh, small_tiles)
    e.kl_step(1, g)
    Wn, Hn, Wp, Hp, allow = oracle_step(X, W, H, wkl, wlh, g)
    assert np.mean(Hp < EPS) >= 0.25 or K == 1, "the step clips too little of H to test anything"
    check(f"{tag}/step/H", e.download_H(), Hn, RT_STEP, pre=Hp, allowance=allow)
    if g < K:
        check(f"{tag}/step/W", e.download_W(), Wn, RT_STEP, pre=Wp)
    else:
        assert np.array_equal(e.download_W(), W)
    for _ in range(run - 2):
        Wn, Hn = (a.T for a in orc.update_WH(X.T, Wn.T, Hn.T, wkl, wlh, g))
    e.kl_step(run - 1, g)
    Wr, Hr, Wp, Hp, allow = oracle_step(X, Wn, Hn, wkl, wlh, g)
    check(f"{tag}/run{run}/H", e.download_H(), Hr, RT_RUN, pre=Hp, allowance=None if allow is None else 8 * allow)
    if g < K:
        check(f"{tag}/run{run}/W", e.download_W(), Wr, RT_RUN, pre=Wp)
    return e


# ------------------------------------------------------------------ the fused per-step pass, every geometry
# K -> (KS, KTM, KR) of salnmf_fused_inst.hip: 1 (1,1,0), 3 (1,1,0), 5 (2,1,0), 8 (2,1,0), 12 (4,1,0), 16 (4,1,0),
# 17-20 (8,1,1-4), 24 (8,2,0), 33-36 (10,2,1-4), 37 (10,3,0), 40 (10,3,0), 41 (13,3,0) ... 48, 49-52 (13,3,1-4), 53 (16,4,0), 64
GEOMETRY_K = [1, 3, 5, 8, 12, 16, 17, 18, 19, 20, 24, 33, 36, 37, 40, 41, 48, 49, 52, 53, 64]


@pytest.mark.parametrize("K", GEOMETRY_K)
def test_fused_step_every_geometry(K):
    N = 16 * (13 + K) + 7  # ragged: the last tile holds 7 samples
    X, W, H = state(96, N, K, seed=100 + K, check_h=K > 1)
    # K = 1: H_new = colsum(X) >= 96 EPSILON, the multiplicative update cannot reach the floor; W can
    step_and_run(f"geom{K}", X, W, H).close()
    if K == 1:  # the floor of H through the l-half root instead (w_lh >> H U / sqrt(EPSILON))
        wlh = 10 ** np.random.default_rng(1).uniform(5.0, 7.0, N)
        step_and_run("geom1/lhalf", X, W, H, wlh=wlh).close()


@pytest.mark.parametrize("N,K", [(16400, 50), (17200, 20)])
def test_cooperative_leftover_tiles(N, K):
    """More tiles than one round of the grid's waves: the leftover round runs as cooperative tiles of four waves."""
    X, W, H = state(96, N, K, seed=N + K)
    step_and_run(f"coop{N}x{K}", X, W, H).close()


@pytest.mark.parametrize("N,K,g", [(50, 3, 0), (200, 8, 0), (333, 12, 2), (1000, 16, 0), (1024, 16, 5)])
def test_small_cohort_kernel(N, K, g):
    """The one-workgroup kernel (salnmf_small.hip): against the oracle entry by entry and against the per-step pass bit for bit."""
    X, W, H = state(96, N, K, seed=N + K, n_given=g)
    b = step_and_run(f"small{N}x{K}g{g}", X, W, H, g=g, small_tiles=64)
    a = engine(X, W, H)
    a.kl_step(1, g), a.kl_step(4, g)
    assert np.array_equal(a.download_W(), b.download_W()) and np.array_equal(a.download_H(), b.download_H())
    a.close(), b.close()


# ------------------------------------------------------------------ weights


def test_weighted_step_wkl():
    N, K = 1500, 24
    wkl = np.random.default_rng(1).uniform(0.5, 2.0, N)
    X, W, H = state(96, N, K, seed=11, wkl=wkl)
    step_and_run("wkl", X, W, H, wkl=wkl).close()


@pytest.mark.parametrize("K", [5, 20, 50])
def test_weighted_step_lhalf_pushes_exposures_to_the_floor(K):
    """l-half weights large enough that the closed-form root sends exposures to the floor; per-entry allowance for
    the cancellation in ``w/2 - sqrt(w^2/4 + i)``."""
    N = 16 * 60 + 5
    rng = np.random.default_rng(K)
    wkl, wlh = rng.uniform(0.5, 2.0, N), rng.uniform(5.0, 60.0, N)
    # (from an unweighted floor state: thirty l-half steps leave too little of W at the floor)
    X, W, H = state(96, N, K, seed=20 + K)
    step_and_run(f"lhalf{K}", X, W, H, wkl=wkl, wlh=wlh).close()
    # without weights_kl: the other branch of the root
    step_and_run(f"lhalf{K}/nokl", X, W, H, wlh=wlh).close()


# ------------------------------------------------------------------ given signatures with entries below the floor


def _given_below_floor(W, g, seed):
    W = W.copy()
    rng = np.random.default_rng(seed)
    for k in range(g):
        cols = rng.choice(W.shape[1], size=12, replace=False)
        W[k, cols[:4]], W[k, cols[4:8]], W[k, cols[8:]] = 0.0, 1e-12, 1e-9
    return W


@pytest.mark.parametrize("K,g", [(8, 3), (20, 3), (50, 7)])
def test_given_signatures_below_the_floor(K, g):
    N = 16 * 40 + 3
    X, W, H = state(96, N, K, seed=60 + K, n_given=g)
    W = _given_below_floor(W, g, K)
    # the joint step clips every row, the given ones too (_utils_klnmf.py:338-341)
    e = step_and_run(f"given{K}g{g}", X, W, H, g=g)
    assert np.array_equal(e.download_W()[:g], W[:g].clip(EPS))
    e.close()
    # update_W with CLIP_NON_GIVEN (:215): the given rows come back as they went in, zeros included
    e = engine(X, W, H)
    e.update_W(g, _lib.CLIP_NON_GIVEN)
    want = orc.update_W(X.T, W.T, H.T, None, g).T
    Wp, _, _, _ = orc.update_WH_preclip(X.T, W.T, H.T, None, None, g)
    Wd = e.download_W()
    assert np.array_equal(Wd[:g], W[:g]) and (Wd[:g] == 0).any()
    check(f"given{K}g{g}/update_W", Wd[g:], want[g:], RT_STEP, pre=Wp.T[g:])
    # CLIP_ALL: the joint step's W tail
    e.upload_W(W)
    e.update_W(g, _lib.CLIP_ALL)
    assert np.array_equal(e.download_W()[:g], W[:g].clip(EPS))
    check(f"given{K}g{g}/update_W_all", e.download_W(), np.clip(Wp.T, EPS, None), RT_STEP, pre=Wp.T)
    # update_H with the given rows' zeros in W
    e.upload_W(W)
    e.update_H()
    _, Hp, _, _ = orc.update_WH_preclip(X.T, W.T, H.T)
    check(f"given{K}g{g}/update_H", e.download_H(), orc.update_H(X.T, W.T, H.T).T, RT_STEP, pre=Hp.T)
    e.close()
    # every signature given: W untouched (not even clipped), H updated
    e = engine(X, W, H)
    e.kl_step(1, K)
    assert np.array_equal(e.download_W(), W)
    _, Hn, _, Hp, _ = oracle_step(X, W, H, g=K)
    check(f"given{K}gK/H", e.download_H(), Hn, RT_STEP, pre=Hp)
    e.close()


# ------------------------------------------------------------------ feature blocks and signature chunks


@pytest.mark.parametrize("V,N,K", [(97, 700, 20), (288, 900, 12), (1536, 400, 10)])
def test_feature_blocks(V, N, K):
    X, W, H = state(V, N, K, seed=V + K)
    if V == 1536:
        assert floor_share(X) >= 0.85  # SBS-1536: about 90 % of the catalogue unobserved
    step_and_run(f"blocks{V}x{K}", X, W, H).close()


@pytest.mark.parametrize("V,N,K", [(96, 900, 65), (96, 700, 130), (288, 500, 130), (97, 600, 65)])
def test_signature_chunks(V, N, K):
    X, W, H = state(V, N, K, seed=V + K + 1)
    step_and_run(f"chunks{V}x{K}", X, W, H, run=3).close()


def test_signature_chunks_given_below_the_floor():
    V, N, K, g = 96, 500, 70, 5
    X, W, H = state(V, N, K, seed=9, n_given=g)
    W = _given_below_floor(W, g, 9)
    e = step_and_run("chunks70g5", X, W, H, g=g, run=2)
    e.close()


# ------------------------------------------------------------------ MvNMF


@pytest.mark.parametrize("V,N,K,g", [(96, 600, 12, 0), (96, 1200, 30, 3), (288, 400, 10, 2)])
def test_mvnmf_step_from_a_floor_state(V, N, K, g):
    lam, delta = 1.0, 1.0
    X, W, H = state(V, N, K, seed=70 + K, n_given=g)
    if g:
        W = _given_below_floor(W, g, K)
    Hm = orc.update_H(X.T, W.T, H.T)
    assert np.mean(orc.update_WH_preclip(X.T, W.T, H.T)[1] < EPS) >= 0.25
    Wn, Hn, gamma = orc.mvnmf_step(X.T, W.T, H.T, lam, delta, 1.0, g)
    Wu = orc.update_W_unconstrained(X.T, W.T, Hm, lam, delta, g)
    e = engine(X, W, H)
    got = e.mv_step(1, g, lam, delta, 1.0)
    assert got == gamma
    # the accepted trial: W_pre = normalised trial before the clip (mvnmf.py:69-92 with gamma = 1: the unconstrained W)
    Wt = Wu if gamma == 1.0 else None
    pre_w = None if Wt is None else (Wt / Wt.sum(axis=0)).T
    check(f"mv{V}x{K}g{g}/W", e.download_W(), Wn.T, RT_MV_W, pre=pre_w)
    pre_h = None if Wt is None else (Hm * Wt.sum(axis=0)[:, None]).T
    check(f"mv{V}x{K}g{g}/H", e.download_H(), Hn.T, RT_MV_H, pre=pre_h)
    e.close()


# ------------------------------------------------------------------ the fp32 fast mode


@pytest.mark.parametrize("N,K", [(700, 16), (900, 36), (17000, 36), (1000, 50), (17000, 8)])
def test_fast_mode_floor(N, K):
    """fp32 steps (salnmf_kernels_f32.h): the floor lands exactly on EPSILON; K = 16 runs ``fused_f32_kernel<4>``,
    K = 33-40 ``<10>``, N = 17 000 more tiles than one round of the grid's waves."""
    X, W, H = state(96, N, K, seed=N + K)
    e = engine(X, W, H)
    e.set_precision("f32")
    e.kl_step(1, 0)
    Wn, Hn, Wp, Hp, _ = oracle_step(X, W, H)
    check(f"f32/{N}x{K}/H", e.download_H(), Hn, RT_F32, pre=Hp, margin=RT_F32)
    check(f"f32/{N}x{K}/W", e.download_W(), Wn, RT_F32, pre=Wp, margin=RT_F32)
    e.close()


# ------------------------------------------------------------------ objectives on floor states


@pytest.mark.parametrize("V,N,K", [(96, 1000, 20), (288, 600, 12), (96, 700, 130)])
def test_objective_and_samplewise_kl_on_floor_states(V, N, K):
    X, W, H = state(V, N, K, seed=V + N + K)
    e = engine(X, W, H)
    assert np.isclose(e.objective(), orc.kl_divergence(X.T, W.T, H.T), rtol=1e-12, atol=0)
    skl = e.samplewise_kl()
    want = orc.samplewise_kl_divergence(X.T, W.T, H.T)
    # all-EPSILON samples have a divergence near 0: an absolute floor per sample, from the size of its terms
    scale = X.sum(axis=1) + (H @ W).sum(axis=1)
    err = np.abs(skl - want)
    assert (err <= 1e-12 * np.abs(want) + SKL_ABS * scale).all(), float(np.max(err / scale))
    _report(f"skl{V}x{K} (abs / scale)", float(np.max(err / scale)))
    e.close()


def test_function_api_where_the_model_is_exactly_zero():
    """All signatures given, channel 0 is 0 in every one of them: P = 0 there and ``tile_kl``'s library branch runs.
    The reference's inf / NaN pattern (tests/golden/kl_floor.npz) must come back."""
    from salamander_amd.models import _utils_klnmf as dev

    fl = np.load(os.path.join(GOLDEN, "kl_floor.npz"))
    assert floor_share(fl["H"]) >= 0.25 and floor_share(fl["W"]) >= 0.25
    Xz, Wz, H = fl["Xz"], fl["Wz"], fl["H"]
    K = Wz.shape[1]
    assert dev.kl_divergence(Xz, Wz, H) == fl["z_kl"] == np.inf
    skl = dev.samplewise_kl_divergence(Xz, Wz, H)
    want = fl["z_skl"]
    assert np.array_equal(np.isinf(skl), np.isinf(want)) and np.array_equal(np.isnan(skl), np.isnan(want))
    fin = np.isfinite(want)
    assert np.allclose(skl[fin], want[fin], rtol=1e-11, atol=1e-11)
    Wn, Hn = dev.update_WH(Xz, Wz, H, None, None, K)
    assert np.array_equal(Wn, Wz)
    for got, ref in ((Hn, fl["z_WH_H"]), (dev.update_H(Xz, Wz, H), fl["z_H"])):
        assert np.array_equal(np.isnan(got), np.isnan(ref)) and np.array_equal(np.isinf(got), np.isinf(ref))
    # and the floor fixture itself through the function-level API, entry by entry
    X, W, H, g = fl["X"], fl["W"], fl["H"], int(fl["n_given"])
    for tag, ng in (("g0", 0), ("g3", g)):
        Wd, Hd = dev.update_WH(X, W, H, None, None, ng)
        Wp, Hp, _, _ = orc.update_WH_preclip(X, W, H, None, None, ng)
        check(f"api/{tag}/W", Wd, fl[f"WH_{tag}_W"], RT_STEP, pre=Wp)
        check(f"api/{tag}/H", Hd, fl[f"WH_{tag}_H"], RT_STEP, pre=Hp)
    Wd = dev.update_W(X, W, H, None, g)
    assert np.array_equal(Wd[:, :g], W[:, :g])
    check("api/W_g3", Wd[:, g:], fl["W_g3"][:, g:], RT_STEP)


# ------------------------------------------------------------------ a trajectory


def test_trajectory_of_fifty_steps_keeps_the_oracles_floor():
    V, N, K = 96, 2000, 20
    X, W0, H0 = orc.sparse_problem(V, N, K, seed=5)
    e = engine(X, W0, H0)
    e.kl_step(49, 0)
    W, H = W0.T, H0.T
    for _ in range(49):
        W, H = orc.update_WH(X.T, W, H)
    e.kl_step(1, 0)
    Wn, Hn, Wp, Hp, _ = oracle_step(X, W.T, H.T)
    assert floor_share(Hn) >= 0.25 and floor_share(Wn) >= 0.25
    Wd, Hd = e.download_W(), e.download_H()
    assert np.array_equal(Hd == EPS, Hn == EPS) and np.array_equal(Wd == EPS, Wn == EPS)
    check("traj50/H", Hd, Hn, RT_TRAJ, pre=Hp)
    check("traj50/W", Wd, Wn, RT_TRAJ, pre=Wp)
    e.close()


# ------------------------------------------------------------------ sample shards (two processes on one GPU)


def _shard_worker(rank, world, port, out_dir):
    sys.path.insert(0, ROOT)
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    import torch.distributed as dist

    from oracle import klnmf_oracle as orc
    from salamander_amd.distributed import attach_peer_exchange, shard_bounds
    from salamander_amd.engine import Engine

    os.environ["MASTER_ADDR"], os.environ["MASTER_PORT"] = "127.0.0.1", str(port)
    dist.init_process_group("gloo", rank=rank, world_size=world)
    try:
        X, W, H = orc.floor_state(96, 2500, 20, seed=31, active=(1, 4))
        a, b = shard_bounds(2500, world, rank)
        e = Engine(b - a, 96, 20)
        e.upload_X(X[a:b]), e.upload_W(W), e.upload_H(H[a:b])
        attach_peer_exchange(e)
        e.kl_step(1, 0)
        W1, H1 = e.download_W(), e.download_H()
        e.kl_step(4, 0)
        np.savez(os.path.join(out_dir, f"rank{rank}.npz"), W1=W1, H1=H1, W5=e.download_W(), H5=e.download_H())
        dist.barrier()
        e.close()
    finally:
        dist.destroy_process_group()


def test_sample_shards_two_ranks(tmp_path):
    import torch.multiprocessing as mp

    from test_distributed_gloo import _free_port

    mp.spawn(_shard_worker, args=(2, _free_port(), str(tmp_path)), nprocs=2, join=True)
    parts = [np.load(os.path.join(tmp_path, f"rank{r}.npz")) for r in range(2)]
    X, W, H = orc.floor_state(96, 2500, 20, seed=31, active=(1, 4))
    assert floor_share(H) >= 0.25 and floor_share(W) >= 0.25
    assert np.array_equal(parts[0]["W1"], parts[1]["W1"]) and np.array_equal(parts[0]["W5"], parts[1]["W5"])
    Wn, Hn, Wp, Hp, _ = oracle_step(X, W, H)
    check("shards/step/W", parts[0]["W1"], Wn, RT_STEP, pre=Wp)
    check("shards/step/H", np.concatenate([p["H1"] for p in parts]), Hn, RT_STEP, pre=Hp)
    for _ in range(3):
        Wn, Hn = (a.T for a in orc.update_WH(X.T, Wn.T, Hn.T))
    Wr, Hr, Wp, Hp, _ = oracle_step(X, Wn, Hn)
    check("shards/run5/W", parts[0]["W5"], Wr, RT_RUN, pre=Wp)
    check("shards/run5/H", np.concatenate([p["H5"] for p in parts]), Hr, RT_RUN, pre=Hp)
