"""CorrNMF embedding solves problem by problem against the host reference (``tests/_ncg_ref.py``).

Every device form of the Newton-CG embedding solves -- the batched sample solves in each of their nine ``(NE, NJ)``
instantiations (``csrc/salnmf_corr_batched.hip``), the one-wavefront-per-sample kernel at one and two terms per lane,
the joint multi-modal solve, the one-workgroup signature kernel and every lockstep evaluation class with its fallback
past ``LS_EVAL_MAX`` evaluations (``csrc/salnmf_host_corr.h``) -- is compared, problem by problem, with the same solver
run on the host with a long-double evaluator.  A problem whose perturbed host ensemble takes one path is *stable*: the
device must reproduce the reference's status and iterate to ``TOL_STABLE`` (or to a twentieth of the ensemble's own
spread where the problem is that ill-conditioned).  An unstable problem must match one run of the ensemble; at most 5 %
of a truncated case may be unstable.  Runs to convergence (``maxiter = 0`` sample solves) end at the solver's noise floor,
where the ensemble itself scatters (tests/_ncg_ref.py: ``envelope``).
"""

import numpy as np
import pytest

import _ncg_ref as nr
from salamander_amd import _lib
from salamander_amd.engine import Engine
from salamander_amd.models import _utils_corrnmf as uc

pytestmark = pytest.mark.gpu

VAR_SAMPLE = 0.8
VAR_SIGNATURE = 1.0


def problem(N, K, dim, seed, spread_L=0.5):
    """Scalings, embeddings and aux (N, K) of a CorrNMF state near its data: aux drawn around the model's exposures."""
    rng = np.random.default_rng(seed)
    alpha = rng.normal(np.log(50.0 / K), 0.5, N)
    beta = rng.normal(0.0, 0.3, K)
    L = rng.normal(0.0, spread_L, (K, dim))
    U = rng.normal(0.0, 0.5, (N, dim))
    aux = rng.gamma(2.0, np.exp(alpha[:, None] + beta[None, :] + U @ L.T) / 2.0)
    return alpha, beta, L, U, aux


def engine(alpha, beta, L, U, aux):
    N, K, dim = U.shape[0], L.shape[0], L.shape[1]
    e = Engine(N, 1, K)
    e.corr_configure(dim)
    e.corr_upload(_lib.CORR_SAMPLE_SCALINGS, alpha)
    e.corr_upload(_lib.CORR_SIGNATURE_SCALINGS, beta)
    e.corr_upload(_lib.CORR_SIGNATURE_EMBEDDINGS, L)
    e.corr_upload(_lib.CORR_SAMPLE_EMBEDDINGS, U)
    e.corr_upload(_lib.CORR_AUX, np.ascontiguousarray(aux))
    return e


def device_samples(alpha, beta, L, U, aux, maxiter, batched=True):
    """More than 64 terms (an engine holds at most 64 signatures): the terms split over modalities of <= 64, joint solve."""
    K = L.shape[0]
    cuts = [(a, min(a + 64, K)) for a in range(0, K, 64)]
    engines = []
    try:
        for a, b in cuts:
            engines.append(engine(alpha, beta[a:b], L[a:b], U, aux[:, a:b]))
            engines[-1].set_batched_sample_solves(batched)
        if len(engines) == 1:
            status = engines[0].corr_update_sample_embeddings(VAR_SAMPLE, maxiter, return_status=True)
        else:
            status = Engine.corr_update_sample_embeddings_multi(engines, VAR_SAMPLE, maxiter, return_status=True)
        return engines[0].corr_download(_lib.CORR_SAMPLE_EMBEDDINGS), status
    finally:
        for e in engines:
            e.close()


def device_signatures(alpha, beta, L, U, aux, lockstep=True):
    e = engine(alpha, beta, L, U, aux)
    try:
        e.set_lockstep(lockstep)
        status = e.corr_update_signature_embeddings(VAR_SIGNATURE, 0, return_status=True)
        return e.corr_download(_lib.CORR_SIGNATURE_EMBEDDINGS), status
    finally:
        e.close()


def check_samples(name, alpha, beta, L, U, aux, maxiter, batched=True, max_unstable=nr.MAX_UNSTABLE):
    x, status = device_samples(alpha, beta, L, U, aux, maxiter, batched)
    assert np.isfinite(x).all()
    off = alpha[:, None] + beta[None, :]
    ref = nr.solve(nr.sample_problems(L, off, aux, U, VAR_SAMPLE, maxiter))
    nr.check(name, ref, x, status, envelope=maxiter <= 0, max_unstable=max_unstable)
    return x, status, ref


def check_signatures(name, alpha, beta, L, U, aux, lockstep=True, max_unstable=nr.MAX_UNSTABLE):
    x, status = device_signatures(alpha, beta, L, U, aux, lockstep)
    assert np.isfinite(x).all()
    ref = nr.solve(nr.signature_problems(U, alpha, beta, aux, L, VAR_SIGNATURE, 0))
    nr.check(name, ref, x, status, max_unstable=max_unstable)
    return x, status, ref


# ------------------------------------------------------------------ batched sample solves: every (NE, NJ) instantiation

# (NE, NJ) = ((terms + 3) // 4, (dim + 3) // 4) rounded up to the first instantiation that covers it, in the order of
# launch_sample_embeddings_batched: (2,2) (4,4) (8,4) (8,8) (16,8) (10,10) (20,10) (12,12) (20,12)
BATCHED = [
    ("2x2", 13, 5, 3, 3),  # N < 16: one wave, three empty slots
    ("2x2", 400, 5, 3, 0),
    ("4x4", 20011, 16, 9, 3),  # > 16 samples per wave on a 256-CU chip: every slot refilled mid-wave
    ("8x4", 777, 24, 13, 3),
    ("8x4", 300, 17, 16, 0),
    ("8x8", 500, 30, 20, 3),
    ("16x8", 301, 50, 24, 3),
    ("10x10", 1000, 40, 40, 3),
    ("20x10", 333, 64, 36, 3),
    ("12x12", 299, 44, 45, 3),
    ("20x12", 317, 72, 46, 3),
    ("20x12", 200, 80, 48, 3),
]


@pytest.mark.parametrize("inst,N,K,dim,maxiter", BATCHED)
def test_batched_sample_solves_per_problem(inst, N, K, dim, maxiter):
    alpha, beta, L, U, aux = problem(N, K, dim, seed=N + K + dim)
    check_samples(f"batched {inst} N={N} K={K} dim={dim} maxiter={maxiter}", alpha, beta, L, U, aux, maxiter)


# ------------------------------------------------------------------ one wavefront per sample (TPL 1 and 2)


@pytest.mark.parametrize(
    "N,K,dim,batched",
    [(300, 40, 40, False), (250, 64, 64, False), (200, 100, 20, False), (211, 90, 10, True), (150, 128, 33, True)],
)
def test_one_wavefront_sample_solves_per_problem(N, K, dim, batched):
    """TPL = 1 (<= 64 terms) and TPL = 2; with batched solves on, terms beyond 80 are handed to this kernel."""
    alpha, beta, L, U, aux = problem(N, K, dim, seed=N + K + dim, spread_L=0.3)
    check_samples(f"one-wave TPL={1 if K <= 64 else 2} N={N} K={K} dim={dim}", alpha, beta, L, U, aux, 3, batched)


# ------------------------------------------------------------------ joint multi-modal sample solves


@pytest.mark.parametrize("Ks,dim,N", [([40, 40], 40, 600), ([10, 20, 15], 12, 500)])
@pytest.mark.parametrize("batched", [True, False])
def test_joint_sample_solves_per_problem(Ks, dim, N, batched):
    rng = np.random.default_rng(sum(Ks) + dim)
    U = rng.normal(0.0, 0.3, (N, dim))
    engines, Ls, offs, auxs = [], [], [], []
    try:
        for K in Ks:
            alpha = rng.normal(np.log(50.0 / K), 0.5, N)
            beta = rng.normal(0.0, 0.3, K)
            L = rng.normal(0.0, 0.3, (K, dim))
            aux = rng.gamma(2.0, np.exp(alpha[:, None] + beta[None, :] + U @ L.T) / 2.0)
            e = engine(alpha, beta, L, U, aux)
            e.set_batched_sample_solves(batched)
            engines.append(e)
            Ls.append(L)
            offs.append(alpha[:, None] + beta[None, :])
            auxs.append(aux)
        status = Engine.corr_update_sample_embeddings_multi(engines, VAR_SAMPLE, 3, return_status=True)
        x = engines[0].corr_download(_lib.CORR_SAMPLE_EMBEDDINGS)
        for e in engines[1:]:
            assert np.array_equal(e.corr_download(_lib.CORR_SAMPLE_EMBEDDINGS), x)
    finally:
        for e in engines:
            e.close()
    ref = nr.solve(nr.sample_problems(np.vstack(Ls), np.hstack(offs), np.hstack(auxs), U, VAR_SAMPLE, 3))
    nr.check(f"joint {Ks} dim={dim} batched={batched}", ref, x, status)


# ------------------------------------------------------------------ signature solves: single kernel and every lockstep class

SIGNATURES = [
    ("one-workgroup", 1500, 7, 8, False),
    ("one-workgroup dim 64", 2100, 4, 64, False),
    ("ls_eval_kernel dim>48", 2100, 5, 56, True),
    ("ls_eval_multi dim%16=0, partial group", 3000, 13, 32, True),
    ("ls_eval_multi dim 16, one group", 2049, 5, 16, True),
    ("packed<3,0> dim 8", 2100, 11, 8, True),
    ("packed<3,0> dim 20", 4100, 7, 20, True),
    ("packed<5,0> dim 12", 2600, 9, 12, True),
    ("packed<5,0> dim 47", 2300, 6, 47, True),
    ("packed<3,40> dim 39", 3100, 12, 39, True),
    ("packed LDS-DMA dim 40", 4100, 8, 40, True),
    ("packed LDS-DMA dim 38", 2051, 13, 38, True),
]


@pytest.mark.parametrize("name,N,K,dim,lockstep", SIGNATURES)
def test_signature_solves_per_problem(name, N, K, dim, lockstep):
    alpha, beta, L, U, aux = problem(N, K, dim, seed=N + K + dim, spread_L=0.3)
    check_signatures(f"{name} N={N} K={K}", alpha, beta, L, U, aux, lockstep)


def test_lockstep_fallback_past_the_evaluation_log():
    """Signature 0 starts 46 units out along every axis (logits up to 216): 218 point evaluations on the host, more than
    LS_EVAL_MAX = 192 -- the single-kernel form finishes it; the other signatures end in lockstep."""
    alpha, beta, L, U, aux = problem(2100, 3, 8, seed=5)
    L[0] += 46.0
    x, _, ref = check_signatures("lockstep fallback N=2100 K=3 dim=8", alpha, beta, L, U, aux)
    assert ref.points[0, 0] > 192 and ref.points[1:, 0].max() < 192


def test_signature_solves_from_gathered_inputs():
    """corr_update_signature_embeddings_from: the engine holds 300 samples, the solves run over all 2 600 handed in."""
    alpha, beta, L, U, aux = problem(2600, 6, 16, seed=11, spread_L=0.3)
    e = engine(alpha[:300], beta, L, U[:300], aux[:300])
    try:
        status = e.corr_update_signature_embeddings_from(U, alpha, aux, VAR_SIGNATURE, 0, return_status=True)
        x = e.corr_download(_lib.CORR_SIGNATURE_EMBEDDINGS)
    finally:
        e.close()
    ref = nr.solve(nr.signature_problems(U, alpha, beta, aux, L, VAR_SIGNATURE, 0))
    nr.check("signatures from gathered inputs N=2600 K=6 dim=16", ref, x, status)


# ------------------------------------------------------------------ edges


def edge_problem(N, K, dim, seed):
    """A zero column of L (that coordinate's optimum is 0: results land on +-EPSILON or 0), offsets below -745 (exp
    underflows to 0) and around +30 (a term that dominates), zero aux columns."""
    alpha, beta, L, U, aux = problem(N, K, dim, seed, spread_L=0.3)
    L[:, dim - 1] = 0.0
    beta[0] = -800.0
    beta[1] = 30.0 - alpha.mean()
    aux[:, 1] = np.exp(30.0 + U @ L[1]) * 0.5
    aux[:, 2] = 0.0
    aux[:, K - 1] = 0.0
    return alpha, beta, L, U, aux


@pytest.mark.parametrize("batched", [True, False])
def test_sample_solve_edges(batched):
    alpha, beta, L, U, aux = edge_problem(700, 12, 6, seed=3)
    check_samples(f"sample edges batched={batched}", alpha, beta, L, U, aux, 3, batched)


@pytest.mark.parametrize("N,lockstep", [(1500, False), (2100, True)])
def test_signature_solve_edges(N, lockstep):
    alpha, beta, L, U, aux = edge_problem(N, 8, 6, seed=4)
    # the same zero column on the sample side: terms = samples, so U[:, 0] = 0 zeroes coordinate 0 of every signature problem
    U[:, 0] = 0.0
    # coordinate 0 converges to rounding noise around 0, which the push turns into +-EPSILON: its sign is a decision a
    # problem may take either way, so most of these problems are unstable and are held to the ensemble
    x, _, _ = check_signatures(f"signature edges N={N} lockstep={lockstep}", alpha, beta, L, U, aux, lockstep, max_unstable=1.0)
    assert (np.abs(x[:, 0]) == nr.EPSILON).sum() >= 3


@pytest.mark.parametrize("batched", [True, False])
def test_dim_one_single_term_sample_solves(batched):
    alpha, beta, L, U, aux = problem(37, 1, 1, seed=7)
    # (one coordinate, one term: three Newton steps reach the optimum and the last line searches work at rounding level)
    check_samples(f"T=1 dim=1 batched={batched}", alpha, beta, L, U, aux, 3, batched, max_unstable=0.25)


@pytest.mark.parametrize("N,lockstep", [(500, False), (2100, True)])
def test_dim_one_signature_solves(N, lockstep):
    alpha, beta, L, U, aux = problem(N, 2, 1, seed=8)
    check_signatures(f"signatures dim=1 N={N} lockstep={lockstep}", alpha, beta, L, U, aux, lockstep, max_unstable=1.0)


def test_update_embedding_single_problems():
    """update_embedding: the sample layout (<= 64 other embeddings), the signature layout (more), an array scaling."""
    rng = np.random.default_rng(9)
    probs, xs = nr.Problems(), []
    for n_other, dim, maxiter in [(1, 1, 3), (7, 3, 3), (64, 16, 0), (65, 8, 0), (300, 5, 3), (2500, 12, 0)]:
        others = rng.normal(0, 0.4, (n_other, dim))
        x0 = rng.normal(0, 0.4, dim)
        scal_other = rng.normal(1.0, 0.3, n_other)
        scaling = rng.normal(0.5, 0.2, n_other) if n_other == 300 else 0.4
        aux = rng.gamma(2.0, np.exp(scaling + scal_other + others @ x0) / 2.0)
        opts = {"options": {"maxiter": maxiter}} if maxiter else {}
        xs.append(uc.update_embedding(x0, others, scaling, scal_other, VAR_SAMPLE, aux, **opts))
        off = (scal_other + scaling) if np.ndim(scaling) else (scaling + scal_other)
        probs.add(probs.matrix(others), off, aux, x0, VAR_SAMPLE, maxiter)
    ref = nr.solve(probs)
    for p, x in enumerate(xs):
        nr.check(f"update_embedding #{p}", nr.subset(ref, [p]), x[None, :], max_unstable=1.0)


# ------------------------------------------------------------------ MultimodalCorrNMF: side-by-side signature solves


def test_side_by_side_signature_solves_equal_sequential():
    from test_gpu_mmcorrnmf import NS_SIGNATURES, DIM_EMBEDDINGS, make_mdata
    from test_oracle_corrnmf import load_mm_case

    import salamander_amd as sal
    from salamander_amd.models.mmcorrnmf import MultimodalCorrNMF

    c = load_mm_case()
    outs = []
    for side in (True, False):
        mdata = make_mdata(c)
        asignatures = {}
        for m in range(2):
            asigs = sal.AnnData(c["Ws"][m].copy())
            asigs.var_names = mdata[f"mod{m}"].var_names
            asigs.obs["scalings"] = c["betas"][m]
            asigs.obsm["embeddings"] = c["Ls"][m].copy()
            asignatures[f"mod{m}"] = asigs
        model = MultimodalCorrNMF(ns_signatures=NS_SIGNATURES, dim_embeddings=DIM_EMBEDDINGS)
        model.mdata, model.asignatures = mdata, asignatures
        model.compute_exposures()
        model.variance = c["variance"]
        model.solve_side_by_side = side
        for _ in range(3):
            model._update_parameters()
        out = [np.array(model.mdata.obsm["embeddings"]), np.array(model.variance)]
        for name in model.mod_names:
            a, s = model.mdata[name], model.asignatures[name]
            out += [np.array(s.X), np.array(s.obs["scalings"]), np.array(s.obsm["embeddings"]), np.array(a.obs["scalings"]), np.array(a.obsm["exposures"])]
        outs.append(out)
    for a, b in zip(*outs):
        assert np.array_equal(a, b)
