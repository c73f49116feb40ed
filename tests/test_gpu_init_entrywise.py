"""The device-side initialisation (``salnmf_init_gram / _project / _finish / _flat / _separable``, ``initialize_on_device``)
entry by entry against ``tests/_init_ref.py``: bit for bit where the arithmetic is exact, within a derived bound against
long double elsewhere, the separable selection's norms within 16 x the float64 replica's measured spread.

(1) Exact-arithmetic inputs, ``np.array_equal``: integer counts (float64 and uint16 upload) for the Gram matrix and the flat
    initialisation, B in sixteenths for the projection and its norms, one-hot rows that hand arbitrary doubles to
    ``init_finish_kernel``.  Shapes name their branch: ragged sample tile, ragged feature tile, feature blocks (the cross-block
    Gram kernels, the projection continued through H), signature chunks (chunk >= 1, the ``first_component`` branch), more
    tiles than workgroups / waves (the grid-stride loops).
(2) Poisson counts clipped to EPSILON with B from the case's own ``eigh``: every entry of the projection and both norms.
(3) ``initialize_on_device`` as a whole on integer counts: signatures bit for bit, every exposure exact or within its bound,
    no entry left out.  The host recipe is handed the norms the device returned (checked against long double first): the
    signatures depend on the bits of the norms (``test_init_ref_host.py::test_signatures_depend_on_the_bits_of_the_norms``).
(4) The separable selection: exact ties (lowest index, in the thread's loop, the 16-slot merge and the selection tree), the
    winning norms, wide rows, the collapse signal.

No tolerance here was chosen from device output; run with ``-s`` for the measured ratios."""

import numpy as np
import pytest

import _init_ref as R
from salamander_amd.device_init import _single_blas_thread, initialize_on_device
from salamander_amd.engine import Engine

pytestmark = pytest.mark.gpu

L = R.L
# measured 2.63e-16 (N=777 V=83 K=12): largest |norm64 - norm_ld| / norm_ld[0], float64 replica in two feature orders against
# the long-double replica, over every round of this file's separable cases.  Each test measures its own inputs' spread on the
# CPU and prints it; it is asserted in test_init_ref_host.py, so that the host's BLAS cannot fail a device test
SEP_SPREAD = 2.7e-16
SEP_TOL = 16 * SEP_SPREAD


def _engine(X, K, dtype=np.float64):
    e = Engine(X.shape[0], X.shape[1], K)
    e.upload_X(np.ascontiguousarray(X.astype(dtype)), clip=False)
    return e


def _mismatch(got, want):
    bad = np.argwhere(np.asarray(got) != np.asarray(want))
    return f"{len(bad)} entries differ, first at {bad[:5].tolist()}: got {[np.asarray(got)[tuple(i)] for i in bad[:3]]}, want {[np.asarray(want)[tuple(i)] for i in bad[:3]]}"


# -------------------------------------------------------------------------------------------------------- (1) exact
@pytest.mark.parametrize("N,V", R.GRAM_SHAPES + [(R.MANY_TILES_N, 96)])
def test_gram_of_integer_counts_is_exact(N, V):
    """(MANY_TILES_N, 96): 1 026 tiles against the 1 024 waves of the Gram launch on 256 compute units (grid = min(compute
    units, ceil(tiles / 4)) workgroups of four waves, salnmf.hip: salnmf_create) -- two waves accumulate a second tile."""
    Xi = R.count_matrix(N, V)
    Gi, total = R.gram_exact(Xi)
    for dtype in (np.float64, np.uint16):
        e = _engine(Xi, 1, dtype)
        G, t = e.init_gram()
        e.close()
        assert np.array_equal(G, G.T), f"{dtype.__name__}: not symmetric"
        assert np.array_equal(G, Gi.astype(np.float64)), f"N={N} V={V} {dtype.__name__}: {_mismatch(G, Gi)}"
        assert t == float(total), (t, total)


@pytest.mark.parametrize("N,V,K", R.PROJECT_SHAPES + [(R.MANY_ROWS, 96, 3)])
def test_projection_in_sixteenths_is_exact(N, V, K):
    Xi = R.count_matrix(N, V)
    B, Bi = R.sixteenths(K, V)
    U, pos2, neg2, bits = R.project_exact(Xi, Bi)
    assert bits <= 53
    e = _engine(Xi, K)
    p, n = e.init_project(B)
    H = e.download_H()
    e.close()
    assert np.array_equal(H, U), f"N={N} V={V} K={K}: {_mismatch(H, U)}"
    assert np.array_equal(p, pos2), _mismatch(p, pos2)
    assert np.array_equal(n, neg2), _mismatch(n, neg2)


@pytest.mark.parametrize("N,V,K", R.FLAT_SHAPES)
def test_flat_of_integer_counts_is_exact(N, V, K):
    Xi = R.count_matrix(N, V)
    post = R.flat_post(K, Xi)
    want = R.flat_replica(Xi, post)
    e = _engine(Xi, K)
    e.init_flat(post)
    H = e.download_H()
    e.close()
    assert np.array_equal(H, want), f"N={N} V={V} K={K}: {_mismatch(H, want)}"
    assert np.array_equal(H[N // 2], np.full(K, R.EPSILON))


@pytest.mark.parametrize("V,K", R.FINISH_SHAPES)
def test_finish_probes_bit_for_bit(V, K):
    """One-hot rows hand B's doubles to H exactly (asserted first); then the finish kernel per element against the replica,
    for fill = 0, 0.25 and a fill whose product with a small post lies below EPSILON.  K = 70: the second chunk starts at global
    column 35 (two chunks of 35); that column and column 64 hold negative probes under take_neg = 0, which must become the fill
    or the floor, never |x| (``first_component`` is chunk 0's alone)."""
    X, B, scale, take_neg, post, perm = R.finish_case(V, K)
    U = B.T[perm]
    e = _engine(X, K)
    for fill in R.FINISH_FILLS:
        e.init_project(B)
        H = e.download_H()
        assert np.array_equal(H, U), f"hand-over V={V} K={K}: {_mismatch(H, U)}"
        e.init_finish(scale, take_neg, post, R.ZERO_BELOW, fill)
        H = e.download_H()
        want = R.finish_replica(U, scale, take_neg, post, R.ZERO_BELOW, fill)
        assert np.array_equal(H, want), f"V={V} K={K} fill={fill}: {_mismatch(H, want)}"
    e.close()


# ---------------------------------------------------------------------------------------------- (2) derived bounds
@pytest.mark.parametrize("N,V,K", R.PROJECT_SHAPES)
def test_projection_entries_and_norms_within_their_bounds(N, V, K):
    X, B = R.generic_case(N, V, K)
    U, a, p, n = R.project_ld(X, B)
    e = _engine(X, K)
    pg, ng = e.init_project(B)
    H = e.download_H()
    e.close()
    ru, rn = R.project_ratios(H, pg, ng, U, a, p, n, N, V)
    print(f"\n[init-entrywise] projection N={N} V={V} K={K}: worst entry {ru * (V + 2):.2f} x 2^-53 a = {ru:.4f} of its bound, worst norm {rn:.4f} of its bound")
    assert np.isfinite(H).all()
    assert ru <= 1.0, f"N={N} V={V} K={K}: an entry of U is {ru:.3f} x its bound (V + 2) 2^-53 a"
    assert rn <= 1.0, f"N={N} V={V} K={K}: a norm is {rn:.3f} x its bound"


# ------------------------------------------------------------------------------------ (3) initialize_on_device as a whole
@pytest.mark.parametrize("V,N,K,method", R.WHOLE_CASES)
def test_whole_device_initialisation_no_entry_left_out(V, N, K, method):
    h = R.WholeHost(V, N, K, method)
    e = _engine(h.X, K)
    G, total = e.init_gram()
    assert np.array_equal(G, h.G) and total == h.total, _mismatch(G, h.G)
    with _single_blas_thread():
        evals, evecs = np.linalg.eigh(G)
    order = np.argsort(evals)[::-1][:K]
    assert np.array_equal(evals[order], h.evals) and np.array_equal(evecs[:, order], h.evecs)  # identical eigenpairs on both sides
    # the norms the device hands the host recipe, against long double
    pd, nd = e.init_project(h.B)
    ratio_n = float((np.maximum(np.abs(pd.astype(L) - h.pos2), np.abs(nd.astype(L) - h.neg2)) / h.bound_n).max())
    assert ratio_n <= 1.0, f"a norm is {ratio_n:.3f} x its bound"
    r = h.recipe(pd, nd)
    r_ld = h.recipe(h.pos2, h.neg2)
    iso = h.isolation(r, pd, nd)
    assert iso["sign"] == 0 and iso["thresh"] == 0 and iso["zero"] == 0 and iso["floor"] == 0 and iso["finite"], iso
    assert np.array_equal(r["take_neg"], r_ld["take_neg"]) and r["fill"] == r_ld["fill"]
    # (scale = lbd / |x|, lbd ~ pos2^(1/4): a relative error d of the norm moves scale by at most d, post by at most d / 2)
    rel = np.maximum(h.bound_n / np.maximum(h.pos2, h.neg2), 0).astype(np.float64) + 16 * R.EPS64
    assert (np.abs(r["scale"] - r_ld["scale"]) <= rel * r_ld["scale"]).all()
    assert (np.abs(r["post"] - r_ld["post"]) <= rel.max() * r_ld["post"]).all()
    # the whole initialisation
    S = initialize_on_device(e, K, method)
    H = e.download_H()
    e.close()
    assert np.array_equal(S, r["S"]), f"signatures: {_mismatch(S, r['S'])}"
    E, exact, bound = h.exposures(r)
    fillv = R.finish_replica(np.zeros((1, K)), r["scale"], r["take_neg"], r["post"], R.ZERO_BELOW, r["fill"])[0]  # float64, as the kernel forms it
    want_exact = np.where(h.scaled(r) < L(R.ZERO_BELOW), fillv[None, :], R.EPSILON)
    assert np.array_equal(H[exact], want_exact[exact]), f"V={V} N={N} K={K} {method}: floor / fill entries: {_mismatch(np.where(exact, H, 0), np.where(exact, want_exact, 0))}"
    err = np.abs(H.astype(L) - E)
    ratio = float((err[~exact] / bound[~exact]).max())
    print(f"\n[init-entrywise] whole V={V} N={N} K={K} {method}: norms {ratio_n:.4f} of their bound; {int(exact.sum())} of {exact.size} exposures exact (floor / fill), "
          f"the others worst {ratio:.4f} of (V + 4) 2^-53 a scale post")
    assert np.array_equal(H[N // 3], want_exact[N // 3]) and exact[N // 3].all()  # the all-zero sample
    assert np.array_equal(H[N - 2], H[1])  # the duplicated sample
    bad = np.argwhere(~exact & (err > bound))
    assert len(bad) == 0, f"V={V} N={N} K={K} {method}: {len(bad)} exposures over their bound, first {bad[:5].tolist()}, worst ratio {ratio:.3f}"


# ----------------------------------------------------------------------------------- (4) the separable selection
def _check_selection(tag, X, K, chosen, norms, rounds=None):
    (c_ld, n_ld, margins), spread = R.separable_spread(X, K)
    rounds = range(K) if rounds is None else rounds
    dev = float(max(abs(float(L(norms[k]) - n_ld[k])) / float(n_ld[0]) for k in rounds))
    print(f"\n[init-entrywise] separable {tag}: host spread {spread:.3g}, device {dev:.3g} of norms[0] (allowed {SEP_TOL:.3g}), smallest lead {margins[list(rounds)].min():.3g}")
    for k in rounds:
        assert margins[k] > 1e-9, (tag, k, margins[k])
        assert chosen[k] == c_ld[k], f"{tag}: round {k} chose {chosen[k]}, the long-double replica {c_ld[k]} (lead {margins[k]:.3g})"
    assert dev <= SEP_TOL, f"{tag}: a winning norm is off by {dev:.3g} of norms[0]"
    return n_ld


@pytest.mark.parametrize("N,V,K", R.SEPARABLE_SHAPES)
def test_separable_indices_and_norms(N, V, K):
    """(150, 250, 10) and (60, 97, 4): ``sep_pass_wide_kernel`` (rows over all feature blocks)"""
    X = R.separable_counts(N, V, K)
    e = _engine(X, K)
    chosen, norms = e.init_separable(K, return_norms=True)
    e.close()
    _check_selection(f"N={N} V={V} K={K}", X, K, chosen, norms)


def test_separable_collapse_signal():
    """The rank-3 catalogue of test_gpu_init.py: rounds 0 - 2 as everywhere else (duplicates tie exactly: lowest index), rounds
    3 - 5 at rounding level, where the norms are compared with nothing but the signal's own threshold."""
    X = R.rank3_catalogue()
    e = _engine(X, 6)
    chosen, norms = e.init_separable(6, return_norms=True)
    e.close()
    _check_selection("rank-3 catalogue", X, 6, chosen, norms, rounds=range(3))
    assert (norms[3:] <= 1e-12 * norms[0]).all() and (norms[3:] >= 0).all(), norms


@pytest.mark.parametrize("variant", sorted(R.TIE_ROWS))
def test_separable_exact_ties_take_the_lowest_index(variant):
    """16 405 rows, 1 024 workgroups of 16 slots (``_init_ref.TIE_ROWS``).  "spread": the copies of the round-0 and of the round-1
    winner sit in different workgroups and slots and in both sweeps of one thread; "last": the lowest copy in workgroup 1023, a
    higher one in workgroup 0 -- the selection tree has to compare indices, not positions; "strided": two workgroups that one
    thread of ``sep_select_kernel`` reduces before the tree, the later one holding the lower row."""
    X, want = R.tie_case(variant)
    e = _engine(X, 3)
    chosen, norms = e.init_separable(2, return_norms=True)
    e.close()
    assert chosen.tolist() == want, (chosen, want)
    _check_selection(f"ties, {variant}", X, 2, chosen, norms)
