"""The exposure covariance's host side without a device: the long-double reference of tests/_cov_ref.py
against mpmath on small problems, the float64 replicas against the reference, closed forms of the contract, the measurement behind
the device tests' tolerances, and every argument ``sal.exposure_covariance`` refuses before it touches a device."""

import mpmath as mp
import numpy as np
import pytest

import _cov_ref as ref
import salamander_amd as sal
import test_gpu_covariance as gpu_tests
from salamander_amd import covariance as cov_mod


def mpmath_contract(x, W, h, idx, information):
    """One sample at 50 digits -> (inflation, standard errors, information diagonal, correlation, smallest squared pivot)"""
    with mp.workdps(50):
        K, V = W.shape
        xs = [max(mp.mpf(float(v)), mp.mpf(ref.EPSILON)) for v in x]
        p = [max(mp.fsum(mp.mpf(float(W[k, v])) * mp.mpf(float(h[k])) for k in range(K)), mp.mpf(ref.EPSILON)) for v in range(V)]
        d = [xs[v] / p[v] ** 2 if information == "observed" else 1 / p[v] for v in range(V)]
        n = len(idx)
        J = mp.matrix(n, n)
        for a, k in enumerate(idx):
            for b, l in enumerate(idx):
                J[a, b] = mp.fsum(mp.mpf(float(W[k, v])) * mp.mpf(float(W[l, v])) * d[v] for v in range(V))
        C = mp.matrix(n, n)
        for a in range(n):
            for b in range(n):
                C[a, b] = J[a, b] / mp.sqrt(J[a, a] * J[b, b])
        L = mp.cholesky(C)
        Ci = mp.inverse(C)
        infl = [Ci[a, a] for a in range(n)]
        corr = np.array([[float(Ci[a, b] / mp.sqrt(Ci[a, a] * Ci[b, b])) for b in range(n)] for a in range(n)])
        return (np.array([float(v) for v in infl]), np.array([float(mp.sqrt(infl[a] / J[a, a])) for a in range(n)]),
                np.array([float(J[a, a]) for a in range(n)]), corr, float(min(L[a, a] ** 2 for a in range(n))))


@pytest.mark.parametrize("information", ["observed", "expected"])
def test_the_reference_against_mpmath(information):
    X, W, H = ref.poisson_case(5, 6, 11, seed=4, mutations=(30, 3000))
    H = ref.restrict_support(H, 4, seed=1)
    H[0] = np.maximum(H[0], 0.5)  # one sample with every signature
    W = ref.normalize(W)
    r = ref.reference(X, W, H, None, information)
    for n in range(5):
        idx = np.flatnonzero(H[n] > 0)
        infl, se, info, corr, piv = mpmath_contract(X[n], W, H[n], idx, information)
        assert np.allclose(np.asarray(r.inflation[n, idx], dtype=float), infl, rtol=1e-14, atol=0)
        assert np.allclose(np.asarray(r.standard_errors[n, idx], dtype=float), se, rtol=1e-14, atol=0)
        assert np.allclose(np.asarray(r.information_diag[n, idx], dtype=float), info, rtol=1e-14, atol=0)
        assert np.allclose(np.asarray(r.correlation[n][np.ix_(idx, idx)], dtype=float), corr, rtol=0, atol=1e-14)
        assert abs(float(r.min_pivot_value[n]) - piv) <= 1e-14
        off = np.abs(corr) - 2.0 * np.eye(idx.size)
        assert np.array_equal(r.most_confounded[n, idx], idx[off.argmax(axis=1)])
        assert np.isnan(np.asarray(r.inflation[n], dtype=float)[H[n] == 0]).all() and (r.most_confounded[n][H[n] == 0] == -1).all()


def test_the_replicas_against_the_reference():
    X, W, H = ref.poisson_case(12, 9, 24, seed=2)
    H = ref.restrict_support(H, 7, seed=2)
    for information in ("observed", "expected"):
        r = ref.reference(X, W, H, None, information)
        assert not r.singular.any() and (r.n_active == 7).all()
        for order, inverse in ref.REPLICAS:
            got = ref.replica(X, W, H, None, information, order=order, inverse=inverse)
            rel, absolute = ref.deviation(got, r)
            print(f"{information} {order} {inverse}: relative {rel:.3g}, absolute {absolute:.3g}, inflation up to {np.nanmax(got.inflation):.3g}")
            # u kappa: the inflation bounds the condition number's part in a diagonal entry of the inverse
            assert rel <= 1e-13 * np.nanmax(got.inflation) and absolute <= 1e-13 * np.nanmax(got.inflation)
            assert np.array_equal(got.most_confounded, r.most_confounded) and np.array_equal(got.singular, r.singular)
            C = got.correlation
            assert np.array_equal(C, C.transpose(0, 2, 1), equal_nan=True)


def test_closed_forms():
    # one signature, observed: J = sum_v w_v^2 x_v / (h w_v)^2 = sum(x) / h^2, so the standard error is h / sqrt(sum x)
    rng = np.random.default_rng(0)
    W = ref.normalize(rng.random((1, 13)) + 0.1)
    X = rng.poisson(40.0, size=(6, 13)).astype(float) + 1.0
    H = rng.uniform(5.0, 500.0, size=(6, 1))
    for fn in (ref.reference, ref.replica):
        r = fn(X, W, H)
        assert np.allclose(np.asarray(r.standard_errors[:, 0], dtype=float), H[:, 0] / np.sqrt(X.sum(axis=1)), rtol=1e-13, atol=0)
        assert (r.inflation == 1.0).all() and (r.min_pivot_value == 1.0).all() and not r.singular.any()
        assert np.isnan(np.asarray(r.max_abs_correlation, dtype=float)).all() and (r.most_confounded == -1).all()
    # disjoint supports: nothing trades against anything
    W = np.zeros((3, 12))
    W[0, :4], W[1, 4:9], W[2, 9:] = rng.random(4) + 0.1, rng.random(5) + 0.1, rng.random(3) + 0.1
    X = rng.poisson(30.0, size=(5, 12)).astype(float)
    H = rng.uniform(1.0, 100.0, size=(5, 3))
    for information in ("observed", "expected"):
        for fn in (ref.reference, ref.replica):
            r = fn(X, W, H, None, information)
            assert (r.inflation == 1.0).all() and (r.max_abs_correlation == 0.0).all() and (r.most_confounded == [1, 0, 0]).all()
    # expected information at the model mean equals the observed one where x = p
    W = ref.signatures(4, 10, seed=1)
    H = rng.uniform(10.0, 100.0, size=(3, 4))
    P = H @ W
    a, b = ref.reference(P, W, H, None, "observed"), ref.reference(P, W, H, None, "expected")
    assert np.allclose(np.asarray(a.standard_errors, dtype=float), np.asarray(b.standard_errors, dtype=float), rtol=1e-12, atol=0)
    # a duplicated signature is singular, with a pivot the reference reports as exactly 0; min_pivot moves the line
    X, W, H = ref.duplicate_case(4, 5, 20, seed=0)
    r = ref.reference(X, W, H)
    assert r.singular.all() and (r.min_pivot_value == 0.0).all() and np.isnan(np.asarray(r.inflation, dtype=float)).all()
    X, W, H = ref.confounded_case(4, 5, 20, seed=0)
    r = ref.reference(X, W, H)
    piv = np.asarray(r.min_pivot_value, dtype=float)
    assert not r.singular.any() and (piv < 0.1).all() and (r.most_confounded[:, 2] == 0).all() and (r.most_confounded[:, 0] == 2).all()
    assert ref.reference(X, W, H, min_pivot=0.5).singular.all()


@pytest.mark.parametrize("case", sorted({k[:-1] for k in gpu_tests.MEASURED}, key=str))
def test_the_recorded_tolerances_hold(case):
    """The device tests give the device 16 times ``MEASURED``: here the four float64 replicas are measured against the reference
    on those tests' own inputs, and none may exceed its record (nor may the record be more than twice what is measured: it is a
    measurement, rounded up).  The same inputs must keep `singular` away from rounding and the partner well defined."""
    name = case[0] if len(case) == 1 else case
    X, W, H, A = gpu_tests.inputs(name)
    for information in ("observed", "expected"):
        r = gpu_tests.reference(name, information)  # (asserts min_pivot_value >= 1e-6 or == 0 on the reference)
        rel, absolute = ref.measure(X, W, H, A, information, ref=r)
        want_rel, want_abs = gpu_tests.MEASURED[(*case, information)]
        print(f"{case} {information}: relative {rel:.3g} (recorded {want_rel:.3g}), absolute {absolute:.3g} (recorded {want_abs:.3g})")
        assert rel <= want_rel <= 2.0 * rel + 1e-300 and absolute <= want_abs <= 2.0 * absolute + 1e-300
        defined = r.most_confounded >= 0
        unclear = defined & ~(np.asarray(r.gap, dtype=float) > 10.0 * gpu_tests.MARGIN * want_abs)
        assert unclear.sum() <= 0.05 * max(1, defined.sum())


class FakeLibrary:
    """Stands where ``libsalnmf.so`` would: records the calls that get past the validation and fills nothing."""

    def __init__(self):
        self.calls = []

    def salnmf_exposure_covariance(self, *args):
        self.calls.append(("covariance", args))
        return 0

    def salnmf_refit_exposures(self, *args):
        self.calls.append(("refit", args))
        for i in range(args[2] * args[5]):  # (the exposures: the covariance call checks what the refit returned)
            args[15][i] = 1.0 + i
        return 0


def test_refusals_come_before_the_library(monkeypatch):
    fake = FakeLibrary()
    monkeypatch.setattr(cov_mod._lib, "load_with_device", lambda: fake)
    X, W, H = ref.poisson_case(4, 3, 10, seed=0)

    def refused(match, *args, **kw):
        with pytest.raises(ValueError, match=match):
            sal.exposure_covariance(*args, **kw)
        assert not fake.calls

    # what the refit refuses of the shared arguments
    refused("1 to 96 signatures, got 97", X, np.ones((97, 10)), np.ones((4, 97)))
    refused("features", X, np.ones((3, 9)), H)
    refused("finite and non-negative", np.where(np.arange(10) == 2, -1.0, X), W, H)
    refused("positive sum", X, np.zeros((3, 10)), H)
    refused("'chunk_bytes'", X, W, H, chunk_bytes=0)
    # its own
    for bad in (np.ones((4, 2)), np.ones((3, 3)), np.ones(3), -H, np.where(H > 50, np.nan, H), np.full((4, 3), np.inf), "abc", H > 1, [["a"] * 3] * 4):
        refused("'exposures' must hold finite numbers >= 0 in shape \\(4, 3\\)", X, W, bad)
    for bad in (np.ones((4, 3)), np.ones(3, dtype=int), [1, 0, 1]):
        refused("'active' must be a boolean array", X, W, H, active=bad)
    for bad in (np.ones((3, 3), dtype=bool), np.ones(4, dtype=bool), np.ones((4, 3, 1), dtype=bool)):
        refused("'active' must have shape \\(3,\\) or \\(4, 3\\)", X, W, H, active=bad)
    for bad in ("fisher", None, 0, b"observed"):
        refused("'information' must be \"observed\" or \"expected\"", X, W, H, information=bad)
    for bad in (0.0, 1.0, -1e-3, 2.0, float("nan"), float("inf"), None, "1e-10", True):
        refused("'min_pivot' must be a finite number in \\(0, 1\\)", X, W, H, min_pivot=bad)
    for bad in (1, None, "yes"):
        refused("'return_correlation' must be True or False", X, W, H, return_correlation=bad)

    # valid calls get as far as the library, with the arguments in the C order
    H0 = H.copy()
    H0[1, 2] = 0.0
    res = sal.exposure_covariance(X, 3.0 * W, H0)
    (kind, args), = fake.calls
    assert kind == "covariance" and args[2:4] == (4, 10) and args[5] == 3 and args[8:11] == (0, 1e-10, 256 << 20) and args[19] is None
    assert np.array_equal(res.active, H0 > 0) and res.active.dtype == bool and not res.active[1, 2] and res.correlation is None
    for name in ("standard_errors", "inflation", "information_diag", "max_abs_correlation", "most_confounded", "exposures", "active"):
        assert getattr(res, name).shape == (4, 3), name
    for name in ("min_pivot_value", "singular", "n_active"):
        assert getattr(res, name).shape == (4,), name
    # the fake library filled nothing
    assert np.isnan(res.standard_errors).all() and (res.most_confounded == -1).all() and res.most_confounded.dtype == np.int32
    assert res.singular.dtype == bool and res.n_active.dtype == np.int32 and res.information == "observed" and res.min_pivot == 1e-10
    assert set(res.timings) == {"information_kernel_ms", "n_chunks", "refit_s", "total_s"}
    mask = np.array([True, False, True])
    res = sal.exposure_covariance(sal.AnnData(X.copy()), W, H, active=mask, information="expected", min_pivot=1e-6, return_correlation=True,
                                  chunk_bytes=4096)
    kind, args = fake.calls[-1]
    assert args[8:11] == (1, 1e-6, 4096) and args[19] is not None and res.correlation.shape == (4, 3, 3)
    assert np.array_equal(res.active, np.broadcast_to(mask, (4, 3))) and res.information == "expected"
    # exposures=None: the refit at its defaults, on the arguments as given, then the covariance at what it returned
    del fake.calls[:]
    res = sal.exposure_covariance(X, W)
    assert [c[0] for c in fake.calls] == ["refit", "covariance"]
    refit_args = fake.calls[0][1]
    assert refit_args[6] == 0 and refit_args[10:14] == (500, 10000, 10, 1e-7)
    assert {"exposure_covariance", "CovarianceResult"} <= set(sal.__all__) and sal.CovarianceResult is cov_mod.CovarianceResult
    assert "observed" in sal.exposure_covariance.__doc__ and "min_pivot" in sal.exposure_covariance.__doc__
