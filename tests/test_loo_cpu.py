"""Leave-one-out cross-validation, CPU side: the NumPy restatement tests/loo_ref.py -- the closed formula against
brute force (N explicit factorizations, the centre held) for all four kernel families, the log densities against the literal formula
of ExactGaussianInference.LOO, the prior at N = 1 --, the surface (header, exports, methods), every refusal that needs no GPU, the
arithmetic of loo_summary and the decision of select_kernels on stub tables, and the seed of the kernel-selection problem.

Bound of formula against brute force: both are fp64 solves with the same Ky, each with a forward error of a modest multiple of
cond(Ky) eps (Cholesky and the triangular solves are backward stable), so they may differ by 10 cond(Ky) eps: absolute in the mean of
O(1) targets, relative to the with-noise variance, relative to 1 + |lpd|.  Measured on this grid (SE; the other families agree at least
as well): 1.7e-16 / 8e-16 at N = 5, 7e-15 / 6e-14 at N = 65, 8e-13 / 1e-12 at N = 129 (noise 1e-3), 8e-12 / 3e-12 at N = 257
(cond 1e6), 4e-9 / 5e-10 at N = 129 with noise 1e-10 (cond 5e7)."""
import ctypes
import os
import re
import sys

import numpy as np
import pytest
from scipy.linalg import lapack

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import loo_ref as LR  # noqa: E402

import bocf_amd as B  # noqa: E402
from bocf_amd import _ffi  # noqa: E402
from oracle import cpu_ref as O  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENTRY_POINTS = ["bocf_loo", "bocf_loo_utility"]
#        N   d  lengthscale noise
GRID = [(5, 2, 0.3, 1e-2), (65, 3, 0.3, 1e-2), (129, 3, 0.5, 1e-3), (257, 6, 0.7, 1e-4), (129, 3, 0.3, 1e-10)]


def _data(N, d, seed=0):
    rng = np.random.RandomState(seed)
    X = rng.uniform(size=(N, d))
    return X, np.sin(3.0 * X.sum(1)) + 0.05 * rng.normal(size=N)


# ---- the restatement ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", LR.FAMILIES)
@pytest.mark.parametrize("N,d,ls,noise", GRID)
def test_formula_against_brute_force(N, d, ls, noise, kind):
    X, y = _data(N, d)
    fit = O.GPFit(kind, X, y, 1.0, np.full(d, ls), noise)
    assert fit.jitter == 0.0
    f = LR.loo_formula_fit(fit, y)
    b = LR.loo_brute(kind, X, y, 1.0, np.full(d, ls), noise)
    bound = 10.0 * np.linalg.cond(LR.train_matrix(kind, X, 1.0, np.full(d, ls), noise)) * np.finfo(float).eps
    dist = LR.distances(f, b, noise) + (LR.distances(f, b, noise, with_noise=False)[1],)
    print("N %d d %d %s: formula vs brute force %s, bound %.1e" % (N, d, kind, ["%.1e" % v for v in dist], bound))
    assert max(dist) <= bound


@pytest.mark.parametrize("kind", ["se", "matern32"])
def test_long_double_brute_force_is_the_fp64_one_to_rounding(kind):
    X, y = _data(33, 2, seed=3)
    b = LR.loo_brute(kind, X, y, 1.3, np.array([0.3, 0.4]), 1e-3)
    t = LR.loo_brute(kind, X, y, 1.3, np.array([0.3, 0.4]), 1e-3, dtype=np.longdouble)
    assert t[0].dtype == np.longdouble
    bound = 10.0 * np.linalg.cond(LR.train_matrix(kind, X, 1.3, np.array([0.3, 0.4]), 1e-3)) * np.finfo(float).eps
    assert max(LR.distances(b, t, 1e-3)) <= bound


def test_one_point_is_the_prior():
    for dtype in (np.float64, np.longdouble):
        mean, var, var0, lpd = LR.loo_brute("matern52", np.array([[0.3, 0.7]]), np.array([1.7]), 2.0, np.array([0.3, 0.3]), 0.25, dtype=dtype)
        assert float(mean[0]) == 1.7                                   # the held centre is the point itself
        np.testing.assert_allclose(np.asarray([var[0], var0[0]], dtype=float), [2.25, 2.0], rtol=1e-15)
        np.testing.assert_allclose(float(lpd[0]), -0.5 * np.log(2 * np.pi * (2.25 + 1e-8)), rtol=1e-15)
    fit = O.GPFit("matern52", np.array([[0.3, 0.7]]), np.array([1.7]), 2.0, np.array([0.3, 0.3]), 0.25)
    f = LR.loo_formula_fit(fit, np.array([1.7]))
    np.testing.assert_allclose([f[0][0], f[1][0], f[2][0]], [1.7, 2.25, 2.0], rtol=1e-15)


@pytest.mark.parametrize("kind", LR.FAMILIES)
def test_lpd_is_the_reference_formula_to_the_letter(kind):
    """exact_gaussian_inference.py:73-79: g = woodbury_vector, c = diag(woodbury_inv) (dpotri of the factor),
    neg_log_marginal_LOO = 0.5 log 2 pi - 0.5 log c + 0.5 g^2 / c, returned negated."""
    X, y = _data(65, 3, seed=1)
    fit = O.GPFit(kind, X, y, 1.0, np.full(3, 0.3), 1e-2)
    Ki = lapack.dpotri(np.asfortranarray(fit.L), lower=1)[0]
    c_diag, g = np.diag(Ki).copy(), fit.alpha[:, 0]
    want = -(0.5 * np.log(2 * np.pi) - 0.5 * np.log(c_diag) + 0.5 * g ** 2 / c_diag)
    f = LR.loo_formula_fit(fit, y)
    np.testing.assert_allclose(f[3], want, rtol=1e-11, atol=0)
    b = LR.loo_brute(kind, X, y, 1.0, np.full(3, 0.3), 1e-2)
    np.testing.assert_allclose(b[3], want, rtol=1e-10, atol=0)        # the Gaussian log density of y_i under the brute-force prediction


def test_expected_utility_restatement():
    rng = np.random.RandomState(5)
    m, n, L, S = 3, 7, 2, 4000
    mean, var = rng.normal(size=(m, n)), rng.uniform(0.05, 0.3, size=(m, n))
    thetas = rng.normal(size=(L, m))
    np.testing.assert_allclose(LR.loo_expected_utility("mean", "linear", thetas, mean, var), thetas.dot(mean))
    Z = rng.normal(size=(L, S, m))
    for kind in ("neg_sq_dist", "neg_sum_exp"):
        closed = LR.loo_expected_utility("closed", kind, thetas, mean, var)
        mc = LR.loo_expected_utility("mc", kind, thetas, mean, var, Z)
        scale = np.abs(closed).max()
        assert np.abs(mc - closed).max() <= 6.0 * scale / np.sqrt(S) * 3.0, kind     # Monte-Carlo error ~ sd / sqrt(S)


# ---- the surface ----------------------------------------------------------------------------------------------------------------
def test_header_declares_and_library_exports_the_entry_points():
    header = open(os.path.join(ROOT, "include", "bocf_hip.h")).read()
    lib = _ffi.load()
    for name in ENTRY_POINTS:
        assert re.search(r"\bint %s\(bocf_ctx\* ctx" % name, header), name
        assert name in _ffi.SIGNATURES
        assert isinstance(getattr(lib, name), ctypes._CFuncPtr)
    from bocf_amd import build
    assert "loo.hip" in build.SOURCES and "capi_loo.hip" in build.SOURCES
    for name in ("loo", "loo_log_likelihood", "loo_summary", "loo_utility", "loo_compare", "select_kernels"):
        assert getattr(B.multi_outputGP, name).__doc__, name
    assert B.CBO.model_check.__doc__


def test_null_context_refusals_name_the_entry_point():
    lib, dp = _ffi.load(), _ffi.dptr
    out, th = np.empty(4), np.zeros((1, 2))

    def bad(rc, name):
        msg = lib.bocf_last_error()
        assert rc < 0 and name.encode() in msg and b"model not fitted" in msg, (rc, msg)
    bad(lib.bocf_loo(None, 3, dp(out), dp(out), dp(out), dp(out)), "bocf_loo")
    bad(lib.bocf_loo(None, 0, None, None, None, None), "bocf_loo")
    bad(lib.bocf_loo_utility(None, 0, 3, _ffi.EU_CLOSED, _ffi.UTIL_NEG_SQ_DIST, None, 0, dp(th), 2, 1, dp(out)), "bocf_loo_utility")


def _stub(m=2, fixed=True):
    model = B.multi_outputGP(m, kernel=[B.kern.SE(2, variance=1.0, lengthscale=0.3) for _ in range(m)], noise_var=[1e-2] * m, fixed_hyps=fixed)
    model._X = np.zeros((3, 2))
    model._Y = [np.zeros((3, 1)) for _ in range(m)]
    return model


def test_python_refusals_without_a_device():
    with pytest.raises(ValueError):
        _stub(fixed=False).loo_compare([[B.kern.SE(2)] * 2])
    with pytest.raises(ValueError):
        _stub(fixed=False).select_kernels([[B.kern.SE(2)] * 2])
    with pytest.raises(ValueError):
        _stub().select_kernels([[B.kern.SE(2)] * 2], criterion="aic")
    with pytest.raises(ValueError):
        _stub().loo_compare([[B.kern.SE(2)]])                          # one kernel for two outputs
    with pytest.raises(RuntimeError):
        B.multi_outputGP(2, fixed_hyps=True).loo_compare([[B.kern.SE(2)] * 2])       # no data yet
    # a utility outside the device set: no host fallback, and nothing touches the device before the refusal
    odd = B.Utility(func=lambda t, y: -np.sum(np.abs(np.asarray(y).T - t).T ** 1.5, axis=0), dfunc=lambda t, y: y,
                    parameter_dist=B.ParameterDistribution(support=np.array([[0.2, 0.1]]), prob_dist=np.ones(1)))
    with pytest.raises(NotImplementedError):
        _stub().loo_utility(odd)


def test_loo_summary_arithmetic():
    Y = np.array([[1.0, 2.0, 3.0, 4.0], [0.0, 0.0, 1.0, 1.0]])
    mean = np.array([[1.5, 2.0, 2.0, 4.0], [0.0, 3.0, 1.0, 1.0]])
    var = np.array([[0.25, 1.0, 0.25, 4.0], [1.0, 1.0, 1.0, 1.0]])
    lpd = np.array([[-1.0, -2.0, -3.0, -4.0], [0.5, 0.5, 0.5, 0.5]])
    s = B.multi_outputGP.loo_summary_of(Y, mean, var, lpd)
    np.testing.assert_allclose(s["lpd"], [-10.0, 2.0])
    np.testing.assert_allclose(s["rmse"], [np.sqrt((0.25 + 1.0) / 4), 1.5])
    z = np.array([[-1.0, 0.0, 2.0, 0.0], [0.0, -3.0, 0.0, 0.0]])
    np.testing.assert_allclose(s["z_mean"], z.mean(1))
    np.testing.assert_allclose(s["z_var"], z.var(1))
    np.testing.assert_allclose(s["coverage"], [0.75, 0.75])
    assert set(s) == {"lpd", "rmse", "z_mean", "z_var", "coverage"}


def test_model_check_is_the_models_summary_and_the_loop_never_asks():
    summary = {"lpd": np.array([1.0])}

    class Model(object):
        def loo_summary(self):
            return summary
    bo = B.CBO.__new__(B.CBO)
    bo.model = Model()
    assert bo.model_check() is summary
    import inspect
    from bocf_amd import cbo
    src = inspect.getsource(cbo)
    assert src.count("model_check") == 1 and src.count("loo_summary") == 2       # the definition; its docstring and its one call


def test_select_kernels_decides_per_output_on_the_table(monkeypatch):
    lists = [[B.kern.SE(2), B.kern.SE(2)], [B.kern.Matern52(2), B.kern.Matern52(2)], [B.kern.Matern32(2), B.kern.Matern32(2)]]
    loo = np.array([[-3.0, -1.0], [-2.0, -5.0], [-2.0, -1.0]])         # output 0: lists 1 and 2 tie -> the earlier; output 1: lists 0 and 2 tie
    lml = np.array([[-9.0, -7.0], [-9.5, -6.0], [-8.0, -6.5]])
    model = _stub()
    seen = []
    monkeypatch.setattr(model, "loo_compare", lambda kl: (seen.append(kl), (loo, lml))[1])
    picked = model.select_kernels(lists)
    assert picked[0] is lists[1][0] and picked[1] is lists[0][1]
    picked = model.select_kernels(lists, criterion="lml")
    assert picked[0] is lists[2][0] and picked[1] is lists[1][1]
    assert len(seen) == 2 and all(len(kl) == 3 for kl in seen)


def test_the_oracle_alone_picks_matern32_on_the_selection_problem():
    """The seed of loo_ref.matern_problem: under both criteria the oracle's tables put matern32 first for both outputs, more than 3 nats
    ahead of the next family -- so the device's pick in tests/test_gpu_loo.py is decided by the data, not by rounding."""
    X, Y, var, ls, noise = LR.matern_problem()
    for table in LR.oracle_tables(X, Y, var, ls, noise):
        order = np.argsort(-table, axis=0)
        assert [LR.FAMILIES[f] for f in order[0]] == ["matern32", "matern32"]
        margin = table[order[0], np.arange(2)] - table[order[1], np.arange(2)]
        assert margin.min() > 3.0, margin
