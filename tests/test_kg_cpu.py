"""Look-ahead posterior and discrete knowledge gradient, CPU side: the NumPy restatement (tests/kg_ref.py) against the oracle's own refit
and its finite differences, the public surface (methods, export, header, library symbols) and uKG's host logic on a mock device model."""
import ctypes
import os
import re
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import kg_ref as K  # noqa: E402

import bocf_amd as B  # noqa: E402
from bocf_amd import _ffi  # noqa: E402
from oracle import cpu_ref as R  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NINE = ["partial_precomputation_for_covariance", "partial_precomputation_for_covariance_gradient",
        "partial_precomputation_for_variance_conditioned_on_next_point", "posterior_variance_conditioned_on_next_point",
        "posterior_variance_gradient_conditioned_on_next_point", "posterior_covariance_between_points_partially_precomputed",
        "posterior_covariance_gradient", "posterior_covariance_gradient_partially_precomputed"]
ENTRY_POINTS = ["bocf_set_ref_points", "bocf_cov_to_ref", "bocf_conditioned_variance", "bocf_acq_kg"]


@pytest.mark.parametrize("kind", ["se", "rbf", "matern52", "matern32"])
@pytest.mark.parametrize("N,noise", [(256, 1e-6), (1024, 1e-6)])
def test_conditioned_variance_equals_the_refit(kind, N, noise):
    """The rank-one downdate of the fit on X equals the oracle's fit on X u {x} (gp.py:514-544 factorizes the bordered Ky): within
    1e-10 sigma_f^2, with no jitter in either fit so the comparison cannot hide behind it.  Includes a next point equal to a training
    input and a query point equal to the next point."""
    d = 3
    X, Y, var, ls, nz, Xc = K.problem([kind], N, d, 40, 5 + N, noise=noise)
    la = K.LookAhead.fit([kind], X, Y, var, ls, nz)
    assert la.fits[0].jitter == 0
    for x in (Xc[:1], X[7:8]):
        P = np.concatenate([Xc[1:], x, X[:3]])
        refit = R.GPFit(kind, np.concatenate([X, x]), np.concatenate([Y[0], [0.3]]).reshape(-1, 1), var[0], ls[0], nz[0])
        assert refit.jitter == 0
        want = refit.raw_posterior_variance(P)[:, 0]
        got = la.conditioned_variance(P, x)[0]
        err = np.max(np.abs(got - want))
        print("conditioned variance vs refit: kind %s N %d max abs difference %.3g (sigma_f^2 = %.3g)" % (kind, N, err, var[0]))
        assert err <= 1e-10 * var[0]


@pytest.mark.parametrize("kind", ["se", "rbf", "matern52", "matern32"])
def test_covariance_equals_predict_full_cov(kind):
    d, N = 2, 120
    X, Y, var, ls, nz, Xc = K.problem([kind], N, d, 30, 3, noise=1e-4)
    la = K.LookAhead.fit([kind], X, Y, var, ls, nz)
    _, full = la.fits[0].predict_full_cov(Xc)
    cov = la.cov(Xc, Xc)[0]
    off = ~np.eye(len(Xc), dtype=bool) & (full > 1e-10)
    assert off.sum() > 100
    np.testing.assert_allclose(cov[off], full[off], rtol=0, atol=1e-10 * var[0])
    # the two halves of the symmetric matrix agree and the diagonal is the raw variance
    np.testing.assert_allclose(cov, cov.T, rtol=0, atol=1e-12)
    np.testing.assert_allclose(np.diag(cov), la.var_raw(Xc)[0], rtol=0, atol=1e-10 * var[0])


def _kg_case(mode, kind):
    kinds = ["se", "matern52", "rbf", "matern32"]
    m = 4 if kind == "rosenbrock" else 3
    d, N, C, na, Sf = 3, 64, 14, 16, 4
    X, Y, var, ls, nz, Xc = K.problem(kinds[:m], N, d, C, 21, noise=1e-4)
    la = K.LookAhead.fit(kinds[:m], X, Y, var, ls, nz)
    rng = np.random.RandomState(4)
    A = rng.uniform(size=(na, d))
    Zf, W = rng.normal(size=(Sf, m)), rng.normal(size=(9, m))
    thetas = rng.uniform(-0.5, 0.5, size=(2, m)) if kind != "rosenbrock" else rng.uniform(0.5, 1.0, size=(2, 1))
    params = rng.uniform(0.5, 1.0, size=m) if kind == "neg_exp_cos" else None
    return la, Xc, A, Zf, W, thetas, np.array([0.3, 0.7]), params


@pytest.mark.parametrize("mode,kind", [("mean", "linear"), ("closed", "neg_sq_dist"), ("closed", "neg_sum_exp"), ("closed", "rosenbrock"),
                                       ("mc", "neg_sq_dist"), ("mc", "neg_exp_cos"), ("mc", "linear")])
def test_kg_gradient_against_finite_differences(mode, kind):
    """The envelope-rule gradient of the restatement agrees with central differences of its own value (rtol 1e-5) on candidates with
    no near tie: best and second-best inner value of every (fantasy, theta) at least 1e-6 max|KG| apart.  At most 5 % of the candidates
    may be left out on these grounds."""
    la, Xc, A, Zf, W, thetas, prob, params = _kg_case(mode, kind)
    r = la.kg(Xc, A, Zf, thetas, prob, mode, kind, W, params, grad=True)
    keep = r["gap"] >= 1e-6 * np.max(np.abs(r["kg"]))
    assert np.mean(~keep) <= 0.05
    h = 1e-5
    fd = np.zeros_like(Xc)
    for q in range(Xc.shape[1]):
        Xp, Xm = Xc.copy(), Xc.copy()
        Xp[:, q] += h
        Xm[:, q] -= h
        fd[:, q] = (la.kg(Xp, A, Zf, thetas, prob, mode, kind, W, params)["kg"] - la.kg(Xm, A, Zf, thetas, prob, mode, kind, W, params)["kg"]) / (2 * h)
    # absolute floor: the rounding of the differences themselves.  Every posterior quantity comes out of triangular solves with the
    # Cholesky factor and carries ~ eps cond(L) = eps sqrt(cond(Ky)) of relative error, cond(Ky) <= (N max sigma_f^2 + nugget) / nugget
    # (1.0e6 here: N = 64, sigma_f^2 <= 1.6, noise 1e-4); KG is a difference of terms of size vscale, so a central difference carries
    # eps sqrt(cond) vscale / h in every component, whatever its own size (2.2e-8 vscale at h = 1e-5; the truncation term is below it)
    atol = np.finfo(float).eps * np.sqrt((64 * 1.6 + 1e-4) / 1e-4) * r["vscale"] / h
    print("KG gradient vs central differences (%s, %s): max abs difference %.3g, gradient scale %.3g, floor %.3g"
          % (mode, kind, np.max(np.abs(r["dkg"][keep] - fd[keep])), np.max(np.abs(fd[keep])), atol))
    np.testing.assert_allclose(r["dkg"][keep], fd[keep], rtol=1e-5, atol=atol)


def test_kg_is_zero_mean_free_for_one_reference_point():
    """With a single reference point and a linear inner value, max_a is the identity and the fantasies enter linearly: KG is exactly
    theta . beta mean(z) -- the restatement's bookkeeping (weights, 1/Sf, v0) in one closed check."""
    kinds = ["se", "rbf"]
    X, Y, var, ls, nz, Xc = K.problem(kinds, 40, 2, 9, 8, noise=1e-4)
    la = K.LookAhead.fit(kinds, X, Y, var, ls, nz)
    rng = np.random.RandomState(1)
    A, Zf, thetas = rng.uniform(size=(1, 2)), rng.normal(size=(5, 2)), rng.normal(size=(3, 2))
    prob = np.array([0.2, 0.5, 0.3])
    got = la.kg(Xc, A, Zf, thetas, prob, "mean", "linear")["kg"]
    beta = la.cov(Xc, A)[:, :, 0] / np.sqrt(la.s2(Xc))
    want = prob.dot(thetas).dot(beta * Zf.mean(0)[:, None])
    np.testing.assert_allclose(got, want, rtol=0, atol=1e-13)


def test_the_model_methods_are_real_and_ukg_is_exported():
    for name in NINE + ["partial_precomputation_for_covariance"]:
        f = getattr(B.multi_outputGP, name)
        assert f is not B.multi_outputGP._off_path, name
        assert f.__doc__
    assert callable(B.multi_outputGP._off_path)
    assert B.uKG is B.acquisitions.uKG and issubclass(B.uKG, B.AcquisitionBase)
    assert B.uKG.analytical_gradient_prediction is True
    model = B.multi_outputGP(2, fixed_hyps=True)
    with pytest.raises(RuntimeError):
        model.partial_precomputation_for_covariance(np.zeros((2, 2)))            # no model yet: a clear error, not NotImplementedError


def test_header_declares_and_library_exports_the_entry_points():
    header = open(os.path.join(ROOT, "include", "bocf_hip.h")).read()
    lib = _ffi.load()
    for name in ENTRY_POINTS:
        assert re.search(r"\bint %s\(bocf_ctx\* ctx" % name, header), name
        i = header.index("int " + name + "(")
        comment = header[header.rfind("/*", 0, i): i]
        assert re.search(r"[a-zA-Z_]+\.py:\d+", comment), "no file:line citation above " + name
        assert name in _ffi.SIGNATURES
        assert isinstance(getattr(lib, name), ctypes._CFuncPtr)
    # argument validation needs no GPU: a null context is refused with the entry point's name
    assert lib.bocf_set_ref_points(None, None, 1) < 0 and b"bocf_set_ref_points" in lib.bocf_last_error()
    assert lib.bocf_cov_to_ref(None, 0, None, None) < 0 and b"bocf_cov_to_ref" in lib.bocf_last_error()
    assert lib.bocf_conditioned_variance(None, 0, 0, None, None) < 0 and b"bocf_conditioned_variance" in lib.bocf_last_error()
    assert lib.bocf_acq_kg(None, 0, 0, None, 0, None, 0, None, 1, None, 1, None, None) < 0 and b"bocf_acq_kg" in lib.bocf_last_error()


# ---- uKG's host logic on a mock device model (the pattern of _MockDeviceModel in tests/test_host_cpu.py)
class _MockKGModel(object):
    analytical_gradient_prediction = True

    def __init__(self, m, d, N=7):
        self.output_dim, self._fit_serial, self.calls = m, 1, []
        self._Xt = np.linspace(0.1, 0.9, N * d).reshape(N, d)

    def number_of_hyps_samples(self):
        return 1

    def _ensure_fitted(self):
        pass

    def get_evaluated_points(self):
        return self._Xt.copy()

    def expected_utility(self, X, mode, utility, thetas, row_param, Z=None, n_hyps=None, grad=False, util_params=None):
        self.calls.append(("eu", mode, utility, np.shape(X), None if Z is None else np.shape(Z)))
        n = len(self._Xt)
        v = np.tile(-np.abs(np.arange(n) - 4.0), len(thetas))                    # training input 4 is the best for every theta
        return v

    def set_reference_points(self, A):
        self.calls.append(("ref", np.array(A)))

    def acq_kg(self, X, mode, util_kind, util_params, thetas, prob, Zf, W=None, n_hyps=None, grad=False, fetch=True):
        self.calls.append(("kg", mode, util_kind, np.array(thetas), None if prob is None else np.array(prob), np.array(Zf),
                           None if W is None else np.array(W), grad))
        X = np.atleast_2d(X)
        v = np.sum(X, 1)
        return (v, np.ones(X.shape)) if grad else v

    def select_topk(self, k):
        return np.arange(k), np.zeros(k)


def _space(d):
    return B.Design_space([{"name": "x%d" % q, "type": "continuous", "domain": (0.0, 1.0)} for q in range(d)])


def test_ukg_host_logic_on_a_mock_device_model():
    m, d = 3, 2
    support = np.array([[0.2, 0.3, 0.5], [0.6, 0.1, 0.3]])
    prob = np.array([0.25, 0.75])
    U = B.Utility(parameter_dist=B.ParameterDistribution(support=support, prob_dist=prob), device="neg_sq_dist")
    model = _MockKGModel(m, d)
    # RNG order: Z_samples (Sf, m), then W_samples (25, m), nothing else with full support
    np.random.seed(11)
    acq = B.uKG(model, _space(d), utility=U, n_fantasies=5, n_ref_points=6)
    after = np.random.uniform()
    np.random.seed(11)
    Z, W = np.random.normal(size=(5, m)), np.random.normal(size=(25, m))
    assert np.random.uniform() == after
    assert np.array_equal(acq.Z_samples, Z) and np.array_equal(acq.W_samples, W)
    assert acq.analytical_gradient_acq
    # first evaluation: reference points drawn (5 uniform + the best training input), staged, mode CLOSED
    X = np.random.uniform(size=(4, d))
    v = acq._compute_acq(X)
    assert v.shape == (4, 1) and np.array_equal(v[:, 0], X.sum(1))
    kinds = [c[0] for c in model.calls]
    assert kinds == ["eu", "ref", "kg"]
    A = model.calls[1][1]
    assert A.shape == (6, d) and np.array_equal(A[-1], model._Xt[4]) and np.all((A >= 0) & (A <= 1))
    kg = model.calls[2]
    assert kg[1] == _ffi.EU_CLOSED and kg[2] == _ffi.UTIL_NEG_SQ_DIST and np.array_equal(kg[3], support) and np.array_equal(kg[4], prob)
    assert np.array_equal(kg[5], Z) and kg[6] is None and kg[7] is False
    # same fit serial: the same set is sent again (free on the device), nothing is redrawn
    state = np.random.get_state()[1].copy()
    v, dv = acq._compute_acq_withGradients(X)
    assert v.shape == (4, 1) and dv.shape == (4, d) and np.array_equal(np.random.get_state()[1], state)
    assert [c[0] for c in model.calls[3:]] == ["ref", "kg"] and np.array_equal(model.calls[3][1], A) and model.calls[4][7] is True
    f, df = acq.acquisition_function_withGradients(X)
    assert np.array_equal(f, -v) and np.array_equal(df, -dv)
    # a new fit serial: drawn and staged again
    model._fit_serial += 1
    n0 = len(model.calls)
    acq._compute_acq(X)
    assert [c[0] for c in model.calls[n0:]] == ["eu", "ref", "kg"] and not np.array_equal(model.calls[n0 + 1][1], A)
    # user-given reference points are used as they are, across refits
    mine = np.random.uniform(size=(3, d))
    acq.set_reference_points(mine)
    model._fit_serial += 1
    n0 = len(model.calls)
    acq._compute_acq(X)
    assert [c[0] for c in model.calls[n0:]] == ["ref", "kg"] and np.array_equal(model.calls[n0][1], mine)
    assert np.array_equal(acq.select_anchors(3), np.arange(3))


def test_ukg_mode_choice_and_missing_device_kind():
    m, d = 4, 2
    dist = B.ParameterDistribution(support=np.array([[0.1, 0.2, 0.3, 0.4]]), prob_dist=np.array([1.0]))
    cases = [(B.Utility(parameter_dist=dist, linear=True, func=lambda t, y: np.dot(t, y)), _ffi.EU_MEAN, _ffi.UTIL_LINEAR),
             (B.Utility(parameter_dist=dist, device="neg_sq_dist"), _ffi.EU_CLOSED, _ffi.UTIL_NEG_SQ_DIST),
             (B.Utility(parameter_dist=dist, device="neg_sum_exp"), _ffi.EU_CLOSED, _ffi.UTIL_NEG_SUM_EXP),
             (B.Utility(parameter_dist=dist, device="rosenbrock"), _ffi.EU_CLOSED, _ffi.UTIL_ROSENBROCK),
             (B.Utility(parameter_dist=dist, device="neg_exp_cos", device_params=np.ones(m)), _ffi.EU_MC, _ffi.UTIL_NEG_EXP_COS)]
    for U, mode, kind in cases:
        model = _MockKGModel(m, d)
        acq = B.uKG(model, _space(d), utility=U, n_fantasies=2, n_ref_points=3)
        assert acq._mode_and_kind() == (mode, kind)
        acq._compute_acq(np.zeros((2, d)))
        kg = model.calls[-1]
        assert kg[1] == mode and kg[2] == kind and (kg[6] is not None) == (mode == _ffi.EU_MC)
        if mode == _ffi.EU_MC:
            assert model.calls[0][4] == (1, 25, m)              # the expected utility of the training inputs uses W as its normals
    odd = B.uKG(_MockKGModel(3, d), _space(d), utility=B.Utility(parameter_dist=B.ParameterDistribution(support=np.array([[0.5]]), prob_dist=np.array([1.0])),
                                                                device="rosenbrock"))
    assert odd._mode_and_kind()[0] == _ffi.EU_MC                   # rosenbrock's closed form needs an even output count
    U = B.Utility(func=lambda t, y: -np.sum(np.abs(y)), dfunc=lambda t, y: -np.sign(y), parameter_dist=dist)
    acq = B.uKG(_MockKGModel(m, d), _space(d), utility=U)
    with pytest.raises(NotImplementedError, match="device kind"):
        acq._compute_acq(np.zeros((2, d)))
    with pytest.raises(ValueError):
        B.uKG(_MockKGModel(m, d), _space(d), utility=U, n_fantasies=0)
