"""The recommendation step of the BOCF loop on the CPU (no GPU): the random draws in the reference's order, the recognition of the
closed-form expectation psi, and the batched L-problem optimiser against a one-parameter-at-a-time restatement of
GeneralOptimizer.optimize, both driven by the oracle's posterior."""
import os
import sys
import warnings

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import bocf_amd as B                                               # noqa: E402
from bocf_amd import recommend as R                                 # noqa: E402
from bocf_amd.acquisition_optimizer import lbfgsb_batched          # noqa: E402
from oracle import cpu_ref as O                                     # noqa: E402


class _ModelStub(object):
    def __init__(self, m, n_samples=10):
        self.output_dim, self._n = m, n_samples

    def number_of_hyps_samples(self):
        return self._n


def _utility(kind, support, prob=None, **kw):
    dist = B.ParameterDistribution(support=np.asarray(support, dtype=float), prob_dist=prob)
    return B.Utility(parameter_dist=dist, device=kind, **kw)


def _space(d, lo=0.0, hi=1.0):
    return B.Design_space([{'name': 'x', 'type': 'continuous', 'domain': (lo, hi), 'dimensionality': d}])


def _restated_draws(seed, support, prob, full, mc, m, bounds, n_starting=200):
    """cbo.py:61-84 (+ :200 in the Monte-Carlo branch) and general_optimizer.py:72-77 -> random_design.py:67-77, as NumPy statements."""
    np.random.seed(seed)
    if full:
        params = support
    else:
        params = support[np.random.choice(len(support), size=10, p=prob), :]
    Z, designs = [], []
    for _ in range(len(params)):
        if mc:
            Z.append(np.random.normal(size=(50, m)))
        X = np.zeros((n_starting, len(bounds)))
        for k in range(len(bounds)):
            X[:, k] = np.random.uniform(low=bounds[k][0], high=bounds[k][1], size=n_starting)
        designs.append(X)
    return params, Z, designs


def _quadratic_factory(parameters, Z):
    """A cheap smooth objective: -||x - c_l||^2 with c_l from the parameter."""
    def ev(X, rows, grad=False):
        c = 0.25 + 0.5 * np.tanh(np.asarray(parameters)[rows, :1])
        diff = X - c
        return -np.sum(diff ** 2, 1), (-2.0 * diff if grad else None)
    return ev


@pytest.mark.parametrize("full", [True, False])
@pytest.mark.parametrize("branch", ["mc", "closed"])
def test_draw_order_matches_the_reference(full, branch):
    m, d = 2, 3
    rng = np.random.RandomState(5)
    support = rng.uniform(-1, 1, size=(4 if full else 25, m))
    prob = np.full(len(support), 1.0 / len(support))
    U = _utility("neg_sq_dist", support, prob)
    psi = B.ExpectationUtility(lambda t, mu, var: R.closed_form("neg_sq_dist", t, mu, var)[0],
                               lambda t, mu, var: R.closed_form("neg_sq_dist", t, mu, var)[1]) if branch == "closed" else None
    space = _space(d, -1.0, 2.0)
    want_params, want_Z, want_designs = _restated_draws(11, support, prob, full, branch == "mc", m, space.get_bounds())
    # what CBO._current_max_value does: the parameter draw (not full support) then the batched recommender
    np.random.seed(11)
    params = support if U.parameter_dist.use_full_support else U.parameter_dist.sample(10)
    assert U.parameter_dist.use_full_support == full
    info = {}
    X, vals = B.current_marginal_argmaxes(_ModelStub(m), space, U, params, psi, evaluator=_quadratic_factory, info=info)
    np.testing.assert_array_equal(params, want_params)
    np.testing.assert_array_equal(info["designs"], np.stack(want_designs))
    if branch == "mc":
        np.testing.assert_array_equal(info["Z"], np.stack(want_Z))
    else:
        assert info["Z"] is None
    assert X.shape == (len(params), d) and vals.shape == (len(params),)
    # and nothing else was drawn: the global stream continues where the restatement's does
    np.random.seed(11)
    _restated_draws(11, support, prob, full, branch == "mc", m, space.get_bounds())
    nxt = np.random.uniform()
    np.random.seed(11)
    params = support if full else U.parameter_dist.sample(10)
    B.current_marginal_argmaxes(_ModelStub(m), space, U, params, psi, evaluator=_quadratic_factory)
    assert np.random.uniform() == nxt


# ---- psi of the forms the reference's experiment scripts use (written afresh here)
def _psi_sq(parameter, mu, var):
    aux = (mu.transpose() - parameter).transpose()
    return -np.sum(np.square(aux), axis=0) - np.sum(var, axis=0)


def _psi_sq_grad(parameter, mu, var):
    mu, var = np.squeeze(mu), np.squeeze(var)
    return -np.concatenate((2 * (mu - parameter), np.ones((len(var),))))


def _psi_exp(parameter, mean, var):
    return -np.sum(np.exp(np.squeeze(mean) + 0.5 * np.squeeze(var)))


def _psi_exp_grad(parameter, mean, var):
    aux = np.exp(np.squeeze(mean) + 0.5 * np.squeeze(var))
    return -np.concatenate((aux, 0.5 * aux))


def _rosen_pair(h):
    def psi(a, mean, var):
        a = float(np.squeeze(a))
        val = 0
        for j in range(h):
            val -= (a - mean[j]) ** 2 + 100 * mean[j + h] ** 2 + var[j] + 100 * var[j + h]
        return val

    def grad(a, mean, var):
        a = float(np.squeeze(a))
        g = np.empty((4 * h,))
        for j in range(h):
            g[j] = 2 * (a - mean[j])
            g[j + h] = -200 * mean[j + h]
            g[j + 2 * h] = -1.
            g[j + 3 * h] = -100.
        return g
    return psi, grad


def _user_utility(kind, support, m):
    """The U of the scripts as a plain callable (recognised by Utility like the reference's)."""
    funcs = {"neg_sq_dist": lambda t, y: -np.sum(np.square((np.asarray(y).T - t).T), axis=0),
             "neg_sum_exp": lambda t, y: np.sum(-np.exp(y), axis=0),
             "rosenbrock": lambda a, y: -(np.sum((np.atleast_1d(a)[0] - np.asarray(y)[:m // 2]) ** 2, axis=0)
                                          + 100 * np.sum(np.asarray(y)[m // 2:] ** 2, axis=0))}
    return B.Utility(func=funcs[kind], dfunc=lambda t, y: O.utility_grad(kind, t, y),
                     parameter_dist=B.ParameterDistribution(support=np.asarray(support, dtype=float), prob_dist=np.ones(len(support)) / len(support)))


@pytest.mark.parametrize("kind,m", [("neg_sq_dist", 2), ("neg_sq_dist", 3), ("neg_sum_exp", 2), ("rosenbrock", 4), ("rosenbrock", 2)])
def test_psi_of_the_scripts_is_recognised_and_a_perturbed_one_is_not(kind, m):
    support = np.array([[0.3, -0.2, 0.1][:m] + [0.0] * max(0, m - 3)]) if kind == "neg_sq_dist" else np.array([[1.0]])
    U = _user_utility(kind, support, m)
    if kind == "neg_sq_dist":
        psi, grad = _psi_sq, _psi_sq_grad
    elif kind == "neg_sum_exp":
        psi, grad = _psi_exp, _psi_exp_grad
    else:
        psi, grad = _rosen_pair(m // 2)
    assert R.recognise_expectation_utility(B.ExpectationUtility(psi, grad), U, m) == kind
    state = np.random.get_state()[1].copy()
    bad_val = B.ExpectationUtility(lambda t, mu, var: psi(t, mu, var) * 1.001, grad)
    bad_grad = B.ExpectationUtility(psi, lambda t, mu, var: np.asarray(grad(t, mu, var)) + 1e-3)
    assert R.recognise_expectation_utility(bad_val, U, m) is None
    assert R.recognise_expectation_utility(bad_grad, U, m) is None
    np.testing.assert_array_equal(np.random.get_state()[1], state)       # the probes use a private RNG
    with warnings.catch_warnings(record=True) as w:
        warnings.simplefilter("always")
        ev = R.make_evaluator(_ModelStub(m), "closed", U, support, bad_val, None, 1)
    assert ev.__qualname__.startswith("host_evaluator") and any("HOST" in str(x.message) for x in w)
    ev = R.make_evaluator(_ModelStub(m), "closed", U, support, B.ExpectationUtility(psi, grad), None, 1)
    assert ev.__qualname__.startswith("device_evaluator")


def test_psi_without_closed_form_kind_is_not_recognised():
    U = _utility("neg_exp_cos", np.array([[0.0]]), np.ones(1), device_params=np.ones(2))
    psi = B.ExpectationUtility(_psi_sq, _psi_sq_grad)
    assert R.recognise_expectation_utility(psi, U, 2) is None


# ---- the batched optimiser against GeneralOptimizer.optimize, one parameter at a time, on the oracle's posterior
def _oracle_model(m, d, N=14, seed=3):
    rng = np.random.RandomState(seed)
    X = rng.uniform(size=(N, d))
    Y = [np.sin(3 * X[:, :1] + j) + 0.3 * X[:, 1:2] * (j + 1) for j in range(m)]
    ref = O.MultiOutputGPRef("rbf", [1.0 + 0.2 * j for j in range(m)], [np.full(d, 0.35 + 0.05 * j) for j in range(m)], [1e-6] * m)
    ref.updateModel(X, Y)
    return ref


def _oracle_factory(ref, branch, kind, n_h, params=None):
    """sum_h E_h[U] of cbo.py:159-231 with the oracle's posterior (fixed hyper-parameters: n_h identical passes)."""
    def factory(parameters, Z):
        def ev(X, rows, grad=False):
            X = np.atleast_2d(X)
            n, d = X.shape
            val, dval = np.zeros(n), np.zeros((n, d))
            for i in range(n):
                # one row at a time: a row's value must not depend on the batch it came in (BLAS blocking does)
                th = parameters[rows[i]]
                mean, var = ref.predict_noiseless(X[i:i + 1])
                if grad:
                    dmean, dvar = ref.posterior_mean_gradient(X[i:i + 1]), ref.posterior_variance_gradient(X[i:i + 1])
                mean, var = np.repeat(mean, n, 1), np.repeat(var, n, 1)
                if grad:
                    dmean, dvar = np.repeat(dmean, n, 1), np.repeat(dvar, n, 1)
                if branch == "closed":
                    v, g = R.closed_form(kind, th, mean[:, i], var[:, i])
                    val[i] = v
                    if grad:
                        dval[i] = g @ np.concatenate((dmean, dvar))[:, i]
                    continue
                std = np.sqrt(var[:, i])
                for z in Z[rows[i]]:
                    y = mean[:, i] + std * z
                    val[i] += O.utility_eval(kind, th, y, params)
                    if grad:
                        dval[i] += O.utility_grad(kind, th, y, params) @ (dmean[:, i, :] + (dvar[:, i, :] / (2 * std)[:, None]) * z[:, None])
            return val * n_h, (dval * n_h if grad else None)
        return ev
    return factory


def _sequential(ev, design, l, bounds, n_anchor=24):
    """GeneralOptimizer.optimize (general_optimizer.py:53-94) for parameter l alone, on the same lbfgsb_batched."""
    rows = np.full(design.shape[0], l)
    scores = -ev(design, rows, False)[0]
    idx = np.argsort(scores, kind="stable")[:n_anchor]
    anchors, avals = design[idx], scores[idx]

    def f_df(X):
        v, g = ev(X, np.full(X.shape[0], l), True)
        return -v, -g
    Xopt, _ = lbfgsb_batched(f_df, anchors, bounds, maxiter=500, factr=1e6)
    fx = np.array([-ev(Xopt[i:i + 1], np.array([l]), False)[0][0] for i in range(len(Xopt))])
    b = int(np.argmin(fx))
    x, f = Xopt[b], fx[b]
    if avals[0] < f:
        x, f = anchors[0], avals[0]
    return anchors, x, f


@pytest.mark.parametrize("branch,kind,m", [("closed", "neg_sq_dist", 2), ("mc", "neg_sq_dist", 2), ("closed", "rosenbrock", 2)])
def test_batched_recommender_matches_one_parameter_at_a_time(branch, kind, m):
    d = 2
    ref = _oracle_model(m, d)
    support = np.array([[0.2, -0.1], [0.6, 0.4], [-0.3, 0.5]]) if kind == "neg_sq_dist" else np.array([[0.5], [1.0], [-0.2]])
    U = _utility(kind, support, np.ones(len(support)) / len(support))
    psi = B.ExpectationUtility(lambda t, mu, var: R.closed_form(kind, t, mu, var)[0],
                               lambda t, mu, var: R.closed_form(kind, t, mu, var)[1]) if branch == "closed" else None
    space = _space(d)
    factory = _oracle_factory(ref, branch, kind, n_h=3)
    np.random.seed(21)
    info = {}
    X, vals = B.current_marginal_argmaxes(_ModelStub(m), space, U, support, psi, n_hyps=3, evaluator=factory, info=info)
    ev = factory(support, info["Z"])
    for l in range(len(support)):
        anchors, x, f = _sequential(ev, info["designs"][l], l, space.get_bounds())
        np.testing.assert_array_equal(info["anchors"][l], anchors)
        np.testing.assert_allclose(X[l], x, rtol=0, atol=1e-8)
        np.testing.assert_allclose(vals[l], -f, rtol=1e-10, atol=1e-12)


def test_cbo_and_helpers_are_exported():
    for name in ("CBO", "Sequential", "MultiObjective", "current_marginal_argmaxes"):
        assert hasattr(B, name), name
    assert callable(getattr(B.multi_outputGP, "expected_utility"))
    assert B.multi_outputGP.expected_utility is not B.multi_outputGP._off_path


def test_multi_objective_draws_one_normal_per_output():
    f = [lambda x: np.sum(x, 1, keepdims=True), lambda x: np.prod(x, 1, keepdims=True)]
    obj = B.MultiObjective(f, noise_var=[0.5, 2.0])
    X = np.array([[0.1, 0.2], [0.3, 0.4]])
    clean, cost = obj.evaluate(X)
    assert cost == 0 and len(clean) == 2 and clean[0].shape == (2, 1)
    np.testing.assert_allclose(obj.evaluate_as_array(X), np.stack([clean[0][:, 0], clean[1][:, 0]]))
    np.random.seed(4)
    noisy, _ = obj.evaluate_w_noise(X)
    np.random.seed(4)
    e0, e1 = np.random.normal(scale=np.sqrt(0.5)), np.random.normal(scale=np.sqrt(2.0))
    np.testing.assert_array_equal(noisy[0], clean[0] + e0)
    np.testing.assert_array_equal(noisy[1], clean[1] + e1)


def test_cbo_refuses_what_it_does_not_provide():
    class Acq(object):
        utility = _utility("neg_sq_dist", np.array([[0.1, 0.2]]), np.ones(1))
    cbo = B.CBO(_ModelStub(2), _space(2), None, Acq(), None, np.zeros((3, 2)))
    with pytest.raises(NotImplementedError):
        cbo._current_max_value_and_var()
    with pytest.raises(NotImplementedError):
        B.CBO(_ModelStub(2), _space(2), None, Acq(), None, np.zeros((3, 2)), cost=lambda x: x)
    cbo.objective = object()
    with pytest.raises(NotImplementedError):
        cbo.run_optimization(1, plot=True)
    with pytest.raises(NotImplementedError):
        cbo.run_optimization(1, context={"x": 0.5})
