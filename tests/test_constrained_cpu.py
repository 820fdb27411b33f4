"""Constrained uEI, CPU side: the NumPy restatement (tests/constrained_ref.py) -- its gradient against central differences of its own
value, the indicator limit, vacuous constraints against the oracle's uEI, the empty feasible set --, OutputConstraints, the public surface
and the refusals of the C ABI that need no GPU."""
import ctypes
import os
import re
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import constrained_ref as CR  # noqa: E402
import kg_ref as K  # noqa: E402

import bocf_amd as B  # noqa: E402
from bocf_amd import _ffi  # noqa: E402
from oracle import cpu_ref as R  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENTRY_POINTS = ["bocf_set_output_constraints", "bocf_feasible_best", "bocf_acq_mc_constrained"]
UTILS = ["linear", "neg_sq_dist", "neg_sum_exp", "neg_exp_cos", "rosenbrock"]


def _small(kind, seed=3, N=14, d=2, m=2, S=40, L=2, n=12, Kc=2, eta=0.05):
    kinds = ["se", "matern52", "rbf", "matern32"][:m]
    X, Y, var, ls, nz, Xc = K.problem(kinds, N, d, n, seed, noise=1e-4)
    la = K.LookAhead.fit(kinds, X, Y, var, ls, nz)
    rng = np.random.RandomState(100 + seed)
    W = rng.normal(size=(S, m))
    thetas, params = CR.utility_inputs(rng, kind, m, L)
    prob = rng.dirichlet(np.ones(L))
    mt = CR.train_mean(la)
    oc = B.OutputConstraints(*CR.draw_constraints(rng, mt, Kc, eta))          # (validated by the public class, as a user's would be)
    return la, Xc, W, thetas, prob, params, mt, oc.A, oc.b, oc.eta


def _alpha(la, X, W, thetas, prob, kind, params, mt, A, b, eta, best=None, grad=False, hard=False):
    post = CR.posterior(la, X, grad=grad)
    return CR.constrained(post[0], post[1], mt, W, thetas, prob, kind, params, A, b, eta, *(post[2:] if grad else ()), best=best, hard=hard)


# ---- the restatement ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", UTILS)
def test_gradient_against_central_differences(kind):
    """The restatement's gradient against central differences of its own value at eta = 0.05, the finite-difference gate of
    test_gpu_round2.py (rtol 1e-3, atol 1e-6 max(1, |g|max)), on the candidates where no sample sits on the hinge: the incumbent is the
    MINIMUM feasible utility here (an input of the restatement), so most samples improve and both terms of the gradient are exercised."""
    la, Xc, W, thetas, prob, params, mt, A, b, eta = _small(kind, seed=5)
    feas = np.all(CR.constraint_values(A, b, mt) <= 0, 0)
    assert feas.any()
    best = (np.array([np.min(R.utility_eval(kind, th, mt[:, feas], params)) for th in thetas]), int(feas.sum()))
    r = _alpha(la, Xc, W, thetas, prob, kind, params, mt, A, b, eta, best=best, grad=True)
    h = 1e-6
    keep = (r["gap"] > 1e-4 * max(r["scale"], 1.0)) & (r["alpha"] > 0)
    assert keep.sum() >= 4
    fd = np.zeros_like(Xc)
    for q in range(Xc.shape[1]):
        Xp, Xm = Xc.copy(), Xc.copy()
        Xp[:, q] += h
        Xm[:, q] -= h
        fd[:, q] = (_alpha(la, Xp, W, thetas, prob, kind, params, mt, A, b, eta, best=best)["alpha"]
                    - _alpha(la, Xm, W, thetas, prob, kind, params, mt, A, b, eta, best=best)["alpha"]) / (2 * h)
    g = r["dalpha"]
    print("%s: gradient vs central differences on %d of %d candidates: max abs difference %.3g, gradient scale %.3g"
          % (kind, keep.sum(), len(Xc), np.abs(g[keep] - fd[keep]).max(), np.abs(g).max()))
    assert np.abs(g[keep]).max() > 0
    np.testing.assert_allclose(g[keep], fd[keep], rtol=1e-3, atol=1e-6 * max(1.0, np.abs(g).max()))


def test_gradient_with_no_feasible_incumbent():
    """F empty: alpha = mean_s phi, and its gradient is that of the smoothed feasibility probability alone."""
    la, Xc, W, thetas, prob, params, mt, A, b, eta = _small("neg_sq_dist", seed=6)
    b = b - 0.3                                                 # a boundary the samples straddle; the empty incumbent is passed by hand
    best = (np.full(len(thetas), -np.inf), 0)
    r = _alpha(la, Xc, W, thetas, prob, "neg_sq_dist", params, mt, A, b, eta, best=best, grad=True)
    np.testing.assert_allclose(r["alpha"], r["phi_mean"] * prob.sum(), rtol=1e-14)
    h, fd = 1e-6, np.zeros_like(Xc)
    for q in range(Xc.shape[1]):
        Xp, Xm = Xc.copy(), Xc.copy()
        Xp[:, q] += h
        Xm[:, q] -= h
        fd[:, q] = (_alpha(la, Xp, W, thetas, prob, "neg_sq_dist", params, mt, A, b, eta, best=best)["alpha"]
                    - _alpha(la, Xm, W, thetas, prob, "neg_sq_dist", params, mt, A, b, eta, best=best)["alpha"]) / (2 * h)
    assert np.abs(r["dalpha"]).max() > 1e-3
    np.testing.assert_allclose(r["dalpha"], fd, rtol=1e-3, atol=1e-6 * max(1.0, np.abs(r["dalpha"]).max()))


@pytest.mark.parametrize("kind", ["neg_sq_dist", "neg_exp_cos"])
def test_indicator_limit(kind):
    """eta = 1e-6: the restatement equals the hard-indicator sum to 1e-12.  Candidates with a sample whose |c_k(y_s)| is below 1e-4 are
    left out of the inputs (s(1e-4 / 1e-6) differs from 1 by e^-100)."""
    la, Xc, W, thetas, prob, params, mt, A, b, _ = _small(kind, seed=7, n=40)
    eta = np.full(len(b), 1e-6)
    probe = _alpha(la, Xc, W, thetas, prob, kind, params, mt, A, b, eta)
    X = Xc[probe["cmin"] >= 1e-4]
    assert len(X) >= 10
    soft = _alpha(la, X, W, thetas, prob, kind, params, mt, A, b, eta)
    hard = _alpha(la, X, W, thetas, prob, kind, params, mt, A, b, eta, hard=True)
    assert soft["cmin"].min() >= 1e-4 and np.any(hard["alpha"] > 0) and np.any((hard["phi_mean"] > 0) & (hard["phi_mean"] < 1))
    np.testing.assert_allclose(soft["alpha"], hard["alpha"], rtol=0, atol=1e-12)


@pytest.mark.parametrize("kind", UTILS)
def test_vacuous_constraints_give_the_oracles_uei(kind):
    la, Xc, W, thetas, prob, params, mt, A, b, eta = _small(kind, seed=8, m=4, L=3)
    mean, var = CR.posterior(la, Xc)
    r = CR.constrained(mean, var, mt, W, thetas, prob, kind, params, A, np.full(len(b), 1e30), eta)
    want, _ = R.mc_acq(mean, np.sqrt(var), mt, W, kind, thetas, prob, "EI", params)
    assert r["n_feasible"] == mt.shape[1] and np.all(r["phi_mean"] == 1.0)
    np.testing.assert_allclose(r["alpha"], want[:, 0], rtol=1e-13, atol=0)


def test_empty_feasible_set_gives_the_mean_of_phi():
    la, Xc, W, thetas, prob, params, mt, A, b, eta = _small("neg_sq_dist", seed=9)
    oc = B.OutputConstraints.bounds(None, [mt[0].min() - 0.2, None], eta=0.05)                 # y_0 <= below every training mean
    A, b, eta = oc.A, oc.b, oc.eta
    assert not oc.feasible(mt).any()
    mean, var = CR.posterior(la, Xc)
    r = CR.constrained(mean, var, mt, W, thetas, None, "neg_sq_dist", params, A, b, eta)
    assert r["n_feasible"] == 0 and np.all(r["best"] == -np.inf)
    y0 = mean[0][None, :] + np.sqrt(var[0])[None, :] * W[:, :1]
    phi = 1.0 / (1.0 + np.exp((y0 - b[0]) / 0.05))
    assert phi.mean(0).max() > 1e-3
    np.testing.assert_allclose(r["alpha"], phi.mean(0), rtol=1e-12)


# ---- OutputConstraints ---------------------------------------------------------------------------------------------------------------
def test_output_constraints_validation_bounds_and_feasible():
    oc = B.OutputConstraints([[1.0, -1.0, 0.0]], [0.5])
    assert (oc.K, oc.m) == (1, 3) and np.array_equal(oc.eta, [1e-3])
    Y = np.array([[0.0, 1.0, 2.0], [0.0, 0.5, 0.0], [9.0, 9.0, 9.0]])
    np.testing.assert_array_equal(oc.feasible(Y), [True, True, False])
    assert oc.feasible(Y[:, 0]) and not oc.feasible(Y[:, 2])
    # bounds: None and infinite entries add no row
    box = B.OutputConstraints.bounds([0.0, None, -np.inf], [1.0, 2.0, None], eta=0.1)
    np.testing.assert_array_equal(box.A, [[1, 0, 0], [-1, 0, 0], [0, 1, 0]])
    np.testing.assert_array_equal(box.b, [1.0, 0.0, 2.0])
    np.testing.assert_array_equal(box.eta, [0.1] * 3)
    np.testing.assert_array_equal(box.feasible(np.array([[0.5, -0.1, 1.0, 0.0], [0.0, 0.0, 2.5, 2.0], [7.0, 7.0, 7.0, -7.0]])), [True, False, False, True])
    np.testing.assert_array_equal(B.OutputConstraints.bounds(None, [1.0, np.inf]).A, [[1.0, 0.0]])
    assert box.key() == B.OutputConstraints(box.A, box.b, box.eta).key() != oc.key()
    for bad in (lambda: B.OutputConstraints(np.zeros((9, 2)), np.zeros(9)),            # K > 8
                lambda: B.OutputConstraints(np.zeros((0, 2)), np.zeros(0)),
                lambda: B.OutputConstraints(np.zeros((2, 2)), np.zeros(3)),            # b shape
                lambda: B.OutputConstraints(np.zeros((2, 2)), np.zeros(2), eta=[0.1, 0.1, 0.1]),
                lambda: B.OutputConstraints(np.zeros((2, 2)), np.zeros(2), eta=0.0),
                lambda: B.OutputConstraints(np.zeros((2, 2)), np.zeros(2), eta=[0.1, -1.0]),
                lambda: B.OutputConstraints(np.zeros((2, 2)), np.zeros(2), eta=np.inf),
                lambda: B.OutputConstraints([[np.nan, 0.0]], [0.0]),
                lambda: B.OutputConstraints([[1.0, 0.0]], [np.inf]),
                lambda: B.OutputConstraints(np.zeros((2, 2, 2)), np.zeros(2)),
                lambda: B.OutputConstraints.bounds([None, None], [np.inf, None]),      # no row at all
                lambda: B.OutputConstraints.bounds([0.0], [1.0, 2.0]),
                lambda: B.OutputConstraints.bounds(None, None),
                lambda: oc.feasible(np.zeros((2, 4)))):
        with pytest.raises(ValueError):
            bad()


# ---- surface ---------------------------------------------------------------------------------------------------------------------
def test_header_declares_and_library_exports_the_entry_points():
    header = open(os.path.join(ROOT, "include", "bocf_hip.h")).read()
    lib = _ffi.load()
    for name in ENTRY_POINTS:
        assert re.search(r"\bint %s\(bocf_ctx\* ctx" % name, header), name
        assert name in _ffi.SIGNATURES
        assert isinstance(getattr(lib, name), ctypes._CFuncPtr)


def test_abi_refusals_that_need_no_gpu():
    lib, dp = _ffi.load(), _ffi.dptr
    A, b, eta = np.ones((2, 3)), np.zeros(2), np.full(2, 0.1)

    def bad(rc, name, text):
        msg = lib.bocf_last_error()
        assert rc < 0 and name.encode() in msg and text.encode() in msg, (rc, msg, text)

    def put(A=A, b=b, eta=eta, K=2, m=3):
        return lib.bocf_set_output_constraints(None, dp(A), dp(b), dp(eta), K, m)
    who = "bocf_set_output_constraints"
    bad(put(K=9), who, "K out of range")
    bad(put(K=-1), who, "K out of range")
    bad(put(m=0), who, "m out of range")
    bad(put(m=17), who, "m out of range")
    bad(put(A=None), who, "null")
    bad(put(A=np.array([[1.0, np.inf, 0.0], [0.0, 0.0, 0.0]])), who, "non-finite")
    bad(put(b=np.array([0.0, np.nan])), who, "non-finite")
    bad(put(eta=np.array([0.1, 0.0])), who, "eta must be finite and > 0")
    bad(put(eta=np.array([-0.1, 0.1])), who, "eta must be finite and > 0")
    bad(put(eta=np.array([np.inf, 0.1])), who, "eta must be finite and > 0")
    bad(put(), who, "null context")
    bad(put(K=0), who, "null context")
    th = np.zeros((1, 3))
    bad(lib.bocf_feasible_best(None, 1, None, 0, dp(th), 3, 1, None, None), "bocf_feasible_best", "model not fitted")
    bad(lib.bocf_acq_mc_constrained(None, 1, None, 0, dp(th), 3, None, 1, None, None), "bocf_acq_mc_constrained", "model not fitted")


class _MockModel(object):
    analytical_gradient_prediction = True

    def __init__(self, m):
        self.output_dim, self.calls = m, []

    def number_of_hyps_samples(self):
        return 1

    def set_output_constraints(self, c):
        self.calls.append(("constraints", c))

    def acq_mc_constrained(self, X, util_kind, util_params, thetas, prob, W=None, n_hyps=None, grad=False, fetch=True):
        self.calls.append(("acq", util_kind, np.array(thetas), None if prob is None else np.array(prob), np.array(W), grad))
        X = np.atleast_2d(X)
        return (X.sum(1), np.ones(X.shape)) if grad else X.sum(1)


def test_exports_class_surface_and_rng_touchpoints():
    assert B.uEI_constrained is B.acquisitions.uEI_constrained and issubclass(B.uEI_constrained, B.uEI_noiseless)
    assert B.OutputConstraints is B.constraints.OutputConstraints
    assert B.uEI_constrained.analytical_gradient_prediction is True
    for name in ("set_output_constraints", "feasible_best", "acq_mc_constrained"):
        assert getattr(B.multi_outputGP, name).__doc__
    from bocf_amd import build
    assert "cacq.hip" in build.SOURCES and "capi_constrained.hip" in build.SOURCES
    model = B.multi_outputGP(2, fixed_hyps=True)
    assert "constraints" in model._resident.__slots__ and model._resident.constraints is None
    with pytest.raises(RuntimeError):
        model.set_output_constraints(B.OutputConstraints([[1.0, 0.0]], [0.0]))          # no model yet: a clear error
    # the same np.random draws as uEI_noiseless, in the constructor and per call
    support = np.array([[0.2, 0.3, 0.5], [0.6, 0.1, 0.3]])
    oc = B.OutputConstraints([[1.0, 0.0, 0.0]], [0.0], eta=0.05)
    out = []
    for cls, kw in ((B.uEI_noiseless, {}), (B.uEI_constrained, {"constraints": oc})):
        for full in (True, False):
            dist = B.ParameterDistribution(support=support if full else np.repeat(support, 10, 0), prob_dist=np.array([0.25, 0.75]) if full else None)
            U = B.Utility(parameter_dist=dist, device="neg_sq_dist")
            np.random.seed(11)
            acq = cls(_MockModel(3) if cls is B.uEI_constrained else _Parent(3), None, utility=U, **kw)
            X = np.random.RandomState(0).uniform(size=(4, 2))
            acq._compute_acq(X)
            acq._compute_acq_withGradients(X)
            out.append((acq.W_samples, np.array(acq.utility_params_samples), np.random.uniform()))
    for a, c in zip(out[:2], out[2:]):
        np.testing.assert_array_equal(a[0], c[0])
        np.testing.assert_array_equal(a[1], c[1])
        assert a[2] == c[2]
    acq, model = _constrained_acq(oc, support)
    X = np.random.RandomState(1).uniform(size=(5, 2))
    v = acq._compute_acq(X)
    assert v.shape == (5, 1) and np.array_equal(v[:, 0], X.sum(1)) and acq.analytical_gradient_acq
    assert [c[0] for c in model.calls] == ["constraints", "acq"] and model.calls[0][1] is oc
    ev = model.calls[1]
    assert ev[1] == _ffi.UTIL_NEG_SQ_DIST and np.array_equal(ev[2], support) and np.array_equal(ev[3], [0.25, 0.75]) and ev[5] is False
    assert np.array_equal(ev[4], acq.W_samples)
    f, df = acq.acquisition_function_withGradients(X)
    assert model.calls[-1][5] is True and np.array_equal(f[:, 0], -X.sum(1)) and np.array_equal(df, -np.ones(X.shape))
    # no host fallback, no utility program, constraints required and of the model's width
    dist = B.ParameterDistribution(support=np.array([[0.1, 0.2, 0.3]]), prob_dist=np.array([1.0]))
    odd = B.uEI_constrained(_MockModel(3), None, utility=B.Utility(func=lambda t, y: -np.sum(np.abs(y)), dfunc=lambda t, y: -np.sign(y), parameter_dist=dist),
                            constraints=oc)
    with pytest.raises(NotImplementedError, match="device kind"):
        odd._compute_acq(X)
    with pytest.raises(NotImplementedError, match="device kind"):
        odd._compute_acq_withGradients(X)
    U = B.Utility(parameter_dist=dist, device="neg_sq_dist")
    with pytest.raises(TypeError):
        B.uEI_constrained(_MockModel(3), None, utility=U)
    with pytest.raises(ValueError):
        B.uEI_constrained(_MockModel(2), None, utility=U, constraints=oc)
    with pytest.raises(TypeError):
        B.uEI_constrained(_Parent(3), None, utility=U, constraints=oc)._compute_acq(X)     # not a device model with the entry point


class _Parent(object):
    """What uEI_noiseless needs of a device model."""
    analytical_gradient_prediction = True

    def __init__(self, m):
        self.output_dim = m

    def number_of_hyps_samples(self):
        return 1

    def acq_linear(self, *a, **kw):
        raise AssertionError("not used")

    def acq_mc(self, X, kind, util_kind, util_params, thetas, prob, W=None, fetch=True, n_hyps=None, program=None):
        return np.zeros(len(np.atleast_2d(X)))

    def acq_mc_grad(self, X, util_kind, util_params, thetas, prob, W=None, n_hyps=None, program=None):
        X = np.atleast_2d(X)
        return np.zeros(len(X)), np.zeros(X.shape)


def _constrained_acq(oc, support):
    U = B.Utility(parameter_dist=B.ParameterDistribution(support=support, prob_dist=np.array([0.25, 0.75])), device="neg_sq_dist")
    model = _MockModel(3)
    np.random.seed(5)
    return B.uEI_constrained(model, None, utility=U, constraints=oc), model
