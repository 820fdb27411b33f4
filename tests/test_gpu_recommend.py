"""The recommendation step on the MI355X: bocf_expected_utility (value and input gradient, every mode x device utility) against a
NumPy restatement of cbo.py:128-231 built on the device model's own per-hyper-sample methods and against the oracle; isolation
from the acquisition state; the Monte-Carlo form against the closed form; and CBO.run_optimization end to end against a loop
written here from the same bocf_amd pieces with the recommendation done on the host, one parameter at a time."""
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import bocf_amd as B                                               # noqa: E402
from bocf_amd import recommend as REC                               # noqa: E402
from bocf_amd.acquisition_optimizer import lbfgsb_batched_numpy    # noqa: E402
from oracle import cpu_ref as O                                     # noqa: E402

pytestmark = pytest.mark.gpu

C_EXPCOS = {1: np.array([0.7]), 2: np.array([0.7, 1.3]), 4: np.array([0.7, 1.3, 0.4, 1.1]), 10: np.linspace(0.4, 1.3, 10)}


def _data(m, d=3, N=30, seed=0):
    rng = np.random.RandomState(seed)
    X = rng.uniform(size=(N, d))
    Y = [(np.sin(3 * X[:, 0] + j) + 0.5 * X[:, 1] * (j + 1) - 0.3 * X[:, 2])[:, None] + 0.01 * rng.normal(size=(N, 1)) for j in range(m)]
    return X, Y


def _fixed_model(m, d=3):
    var = [1.0 + 0.3 * j for j in range(m)]
    ls = [np.full(d, 0.4 + 0.05 * j) for j in range(m)]
    model = B.multi_outputGP(m, kernel=[B.kern.RBF(d, variance=var[j], lengthscale=ls[j], ARD=True) for j in range(m)], noise_var=[1e-4] * m,
                             fixed_hyps=True)
    X, Y = _data(m, d)
    model.updateModel(X, Y)
    ref = O.MultiOutputGPRef("rbf", var, ls, [1e-4] * m)
    ref.updateModel(X, Y)
    return model, ref


def _learned_model(m, d=3, H=10):
    np.random.seed(7 + m)
    model = B.multi_outputGP(m, exact_feval=[True] * m, fixed_hyps=False, n_samples=H)
    model.n_burnin, model.subsample_interval, model.leapfrog_steps = 20, 2, 5
    X, Y = _data(m, d)
    model.updateModel(X, Y)
    return model


_MODELS = {}


def _model(kind, m):
    if (kind, m) not in _MODELS:
        _MODELS[(kind, m)] = _fixed_model(m)[0] if kind == "fixed" else _learned_model(m)
    return _MODELS[(kind, m)]


def _thetas(kind, m, L):
    rng = np.random.RandomState(11 * m + L)
    if kind == "rosenbrock":
        return rng.uniform(0.2, 1.2, size=(L, 1))
    if kind in ("neg_sum_exp", "neg_exp_cos"):
        return rng.uniform(-1, 1, size=(L, 1))
    return rng.uniform(-1, 1, size=(L, m))


def _ueval(kind, th, y, params):
    """U over y (m, ...) -> (...)."""
    th = np.atleast_1d(th)
    if kind == "linear":
        return np.tensordot(th, y, axes=(0, 0))
    if kind == "neg_sq_dist":
        return -np.sum((y - th.reshape((-1,) + (1,) * (y.ndim - 1))) ** 2, 0)
    if kind == "neg_sum_exp":
        return -np.sum(np.exp(y), 0)
    if kind == "neg_exp_cos":
        return -np.tensordot(params, np.exp(-y / np.pi) * np.cos(np.pi * y), axes=(0, 0))
    h = y.shape[0] // 2
    return -(np.sum((th[0] - y[:h]) ** 2, 0) + 100.0 * np.sum(y[h:2 * h] ** 2, 0))


def _ugrad(kind, th, y, params):
    """dU/dy over y (m, ...) -> (m, ...)."""
    th = np.atleast_1d(th)
    sh = (-1,) + (1,) * (y.ndim - 1)
    if kind == "linear":
        return np.broadcast_to(th.reshape(sh), y.shape).copy()
    if kind == "neg_sq_dist":
        return -2.0 * (y - th.reshape(sh))
    if kind == "neg_sum_exp":
        return -np.exp(y)
    if kind == "neg_exp_cos":
        e = np.exp(-y / np.pi)
        return params.reshape(sh) * (np.pi * e * np.sin(np.pi * y) + e * np.cos(np.pi * y) / np.pi)
    h = y.shape[0] // 2
    g = np.zeros_like(y)
    g[:h] = 2.0 * (th[0] - y[:h])
    g[h:2 * h] = -200.0 * y[h:2 * h]
    return g


def _restated(model, X, mode, kind, thetas, rows, Z, n_h, params=None, grad=True):
    """cbo.py:128-231 over the model's public per-h methods (set_hyperparameters(h), predict_noiseless / posterior_mean and the two
    gradients), vectorised over the points (and the samples).  With fixed hyper-parameters the n_h passes are identical: one pass
    counted n_h times."""
    X = np.atleast_2d(X)
    n, d = X.shape
    val, dval = np.zeros(n), np.zeros((n, d))
    hs, w = (range(n_h), 1.0) if not getattr(model, "fixed_hyps", True) else ([0], float(n_h))
    for l in np.unique(rows):
        sel = np.flatnonzero(rows == l)
        Xl, th = X[sel], thetas[l]
        for h in hs:
            model.set_hyperparameters(h)
            if mode == "mean":
                mu = model.posterior_mean(Xl)
                val[sel] += w * np.tensordot(th, mu, axes=(0, 0))
                if grad:
                    dval[sel] += w * np.tensordot(th, model.posterior_mean_gradient(Xl), axes=(0, 0))
                continue
            mean, var = model.predict_noiseless(Xl)
            if grad:
                dmean, dvar = model.posterior_mean_gradient(Xl), model.posterior_variance_gradient(Xl)
            if mode == "closed":
                for i, r in enumerate(sel):
                    v, g = REC.closed_form(kind, th, mean[:, i], var[:, i])
                    val[r] += w * v
                    if grad:
                        dval[r] += w * (g @ np.concatenate((dmean, dvar))[:, i])
                continue
            std = np.sqrt(var)
            y = mean[:, :, None] + std[:, :, None] * Z[l].T[:, None, :]           # (m, n_l, S)
            val[sel] += w * _ueval(kind, th, y, params).sum(-1)
            if grad:
                g = _ugrad(kind, th, y, params)                                    # (m, n_l, S)
                A, Bz = g.sum(-1), (g * Z[l].T[:, None, :]).sum(-1)
                dval[sel] += w * (np.einsum("ji,jiq->iq", A, dmean) + np.einsum("ji,jiq->iq", Bz / (2 * std), dvar))
    return val, dval


def _cases(m):
    out = [("mean", "linear")]
    out += [("closed", k) for k in ("neg_sq_dist", "neg_sum_exp", "rosenbrock") if k != "rosenbrock" or m % 2 == 0]
    out += [("mc", k) for k in ("linear", "neg_sq_dist", "neg_sum_exp", "neg_exp_cos", "rosenbrock") if k != "rosenbrock" or m % 2 == 0]
    return out


@pytest.mark.parametrize("hyp", ["fixed", "learned"])
@pytest.mark.parametrize("m", [1, 2, 4])
def test_expected_utility_matches_restatement_and_separate_calls(hyp, m):
    _check_against_restatement(_model(hyp, m), m)


def test_expected_utility_generic_output_count():
    """m = 10 takes the kernel instantiation whose output count is a run-time argument (m > 8)."""
    _check_against_restatement(_model("fixed", 10), 10)


def _check_against_restatement(model, m):
    rng = np.random.RandomState(3)
    L, n, S = 3, 11, 50
    X = rng.uniform(size=(n, 3))
    rows = rng.randint(0, L, size=n)
    rows[:L] = np.arange(L)                                                       # every parameter present, mixed across rows
    Z = rng.normal(size=(L, S, m))
    n_h = 10
    for mode, kind in _cases(m):
        th = _thetas(kind, m, L) if mode != "mean" else _thetas("linear", m, L)
        params = C_EXPCOS[m] if kind == "neg_exp_cos" else None
        v, g = model.expected_utility(X, mode, kind, th, rows, Z=Z, n_hyps=n_h, grad=True, util_params=params)
        v0 = model.expected_utility(X, mode, kind, th, rows, Z=Z, n_hyps=n_h, grad=False, util_params=params)
        if not model.fixed_hyps:
            assert model._current_h == n_h - 1
        np.testing.assert_allclose(v0, v, rtol=1e-12, atol=1e-300, err_msg="%s %s value-only" % (mode, kind))
        for l in range(L):
            sel = np.flatnonzero(rows == l)
            vs, gs = model.expected_utility(X[sel], mode, kind, th[l:l + 1], np.zeros(len(sel), dtype=int), Z=Z[l:l + 1], n_hyps=n_h, grad=True,
                                            util_params=params)
            np.testing.assert_allclose(vs, v[sel], rtol=1e-12, atol=1e-13 * np.abs(v).max(), err_msg="%s %s separate" % (mode, kind))
            np.testing.assert_allclose(gs, g[sel], rtol=1e-12, atol=1e-12 * np.abs(g).max(), err_msg="%s %s separate grad" % (mode, kind))
        rv, rg = _restated(model, X, mode, kind, th, rows, Z, n_h, params)
        np.testing.assert_allclose(v, rv, rtol=1e-10, atol=1e-11 * np.abs(rv).max(), err_msg="%s %s value" % (mode, kind))
        np.testing.assert_allclose(g, rg, rtol=1e-10, atol=1e-10 * np.abs(rg).max(), err_msg="%s %s gradient" % (mode, kind))


def test_expected_utility_matches_oracle_fixed_hyps():
    m = 2
    model, ref = _fixed_model(m)
    rng = np.random.RandomState(5)
    L, n = 2, 9
    X = rng.uniform(size=(n, 3))
    rows = np.arange(n) % L
    Z = rng.normal(size=(L, 50, m))
    for mode, kind in _cases(m):
        th = _thetas(kind if mode != "mean" else "linear", m, L)
        params = C_EXPCOS[m] if kind == "neg_exp_cos" else None
        v, g = model.expected_utility(X, mode, kind, th, rows, Z=Z, n_hyps=1, grad=True, util_params=params)
        rv, rg = _restated(ref, X, mode, kind, th, rows, Z, 1, params)
        np.testing.assert_allclose(v, rv, rtol=1e-9, atol=1e-9 * np.abs(rv).max(), err_msg="%s %s" % (mode, kind))
        np.testing.assert_allclose(g, rg, rtol=1e-9, atol=1e-9 * np.abs(rg).max(), err_msg="%s %s grad" % (mode, kind))


def test_expected_utility_gradients_match_finite_differences():
    m = 2
    model = _model("fixed", m)
    rng = np.random.RandomState(9)
    n, L = 5, 2
    X = rng.uniform(0.2, 0.8, size=(n, 3))
    rows = np.arange(n) % L
    Z = rng.normal(size=(L, 50, m))
    eps = 1e-5
    for mode, kind in _cases(m):
        th = _thetas(kind if mode != "mean" else "linear", m, L)
        params = C_EXPCOS[m] if kind == "neg_exp_cos" else None
        _, g = model.expected_utility(X, mode, kind, th, rows, Z=Z, n_hyps=3, grad=True, util_params=params)
        fd = np.zeros_like(g)
        for q in range(3):
            E = np.zeros_like(X)
            E[:, q] = eps
            vp = model.expected_utility(X + E, mode, kind, th, rows, Z=Z, n_hyps=3, util_params=params)
            vm = model.expected_utility(X - E, mode, kind, th, rows, Z=Z, n_hyps=3, util_params=params)
            fd[:, q] = (vp - vm) / (2 * eps)
        np.testing.assert_allclose(g, fd, rtol=1e-5, atol=1e-6 * max(1.0, np.abs(g).max()), err_msg="%s %s" % (mode, kind))


def test_expected_utility_leaves_acquisition_state_alone():
    m = 2
    model = _model("fixed", m)
    rng = np.random.RandomState(2)
    X = rng.uniform(size=(300, 3))
    W = rng.normal(size=(25, m))
    th = np.array([[0.3, -0.2], [0.1, 0.5]])
    prob = np.array([0.4, 0.6])
    a1 = model.acq_mc(X, B._ffi.ACQ_EI, B._ffi.UTIL_NEG_SQ_DIST, None, th, prob, W=W)
    i1, v1 = model.select_topk(16)
    a2 = model.acq_mc(X, B._ffi.ACQ_EI, B._ffi.UTIL_NEG_SQ_DIST, None, th, prob, W=W)
    # the expected utility over the SAME resident candidates (X=None), with gradients and its own samples and parameters
    model.expected_utility(None, "mc", "neg_exp_cos", np.zeros((3, 1)), np.arange(300) % 3, Z=rng.normal(size=(3, 50, m)), n_hyps=4, grad=True,
                           util_params=C_EXPCOS[m])
    i2, v2 = model.select_topk(16)
    np.testing.assert_array_equal(a1, a2)
    np.testing.assert_array_equal(i1, i2)
    np.testing.assert_array_equal(v1, v2)
    # the resident W, parameters and best-so-far are those of before: an acquisition on the resident batch without re-sending W
    a3 = model._acq_mc_resident(B._ffi.ACQ_EI, B._ffi.UTIL_NEG_SQ_DIST, None, th, prob, 300)
    np.testing.assert_array_equal(a1, a3)


def test_monte_carlo_form_converges_to_closed_form():
    m = 2
    model = _model("fixed", m)
    rng = np.random.RandomState(4)
    X = rng.uniform(size=(6, 3))
    S = 20000
    for kind in ("neg_sq_dist", "neg_sum_exp", "rosenbrock"):
        th = _thetas(kind, m, 1)
        Z = rng.normal(size=(1, S, m))
        rows = np.zeros(len(X), dtype=int)
        mc = model.expected_utility(X, "mc", kind, th, rows, Z=Z, n_hyps=1) / S
        cf = model.expected_utility(X, "closed", kind, th, rows, n_hyps=1)
        mean, var = model.predict_noiseless(X)
        y = mean[:, :, None] + np.sqrt(var)[:, :, None] * Z[0].T[:, None, :]
        se = _ueval(kind, th[0], y, None).std(-1) / np.sqrt(S)
        assert np.all(np.abs(mc - cf) <= 4 * se + 1e-12), (kind, mc, cf, se)


def test_expected_utility_argument_checks():
    model = _model("fixed", 2)
    X = np.random.RandomState(1).uniform(size=(4, 3))
    th = np.zeros((2, 2))
    with pytest.raises(B._ffi.BocfHipError, match="closed-form"):
        model.expected_utility(X, "closed", "neg_exp_cos", th, np.zeros(4, dtype=int), util_params=C_EXPCOS[2])
    with pytest.raises(B._ffi.BocfHipError, match="closed-form"):
        model.expected_utility(X, "closed", "linear", th, np.zeros(4, dtype=int))
    with pytest.raises(B._ffi.BocfHipError, match="row_param"):
        model.expected_utility(X, "closed", "neg_sq_dist", th, np.array([0, 1, 2, 0]))
    with pytest.raises(B._ffi.BocfHipError, match="fewer"):
        model.expected_utility(X, "mc", "neg_sq_dist", th, np.zeros(4, dtype=int), Z=np.zeros((1, 10, 2)))
    with pytest.raises(B._ffi.BocfHipError, match="theta_dim"):
        model.expected_utility(X, "mean", None, np.zeros((2, 3)), np.zeros(4, dtype=int))
    with pytest.raises(ValueError, match="2-D"):
        model.expected_utility(X, "closed", "neg_sum_exp", np.zeros(2), np.zeros(4, dtype=int))
    model.expected_utility(X, "closed", "neg_sq_dist", th, np.zeros(4, dtype=int))            # 4 candidates now resident
    for bad in (np.zeros(3, dtype=int), np.zeros(5, dtype=int)):
        with pytest.raises(ValueError, match="resident"):
            model.expected_utility(None, "closed", "neg_sq_dist", th, bad)
    assert model.expected_utility(None, "closed", "neg_sq_dist", th, np.zeros(4, dtype=int)).shape == (4,)
    learned = _model("learned", 2)
    with pytest.raises(IndexError):
        learned.expected_utility(X, "closed", "neg_sq_dist", th, np.zeros(4, dtype=int), n_hyps=11)
    learned.updateModel(learned._X, learned._Y)                                               # a refit forgets the resident batch
    with pytest.raises(ValueError, match="resident"):
        learned.expected_utility(None, "closed", "neg_sq_dist", th, np.zeros(4, dtype=int))
    _MODELS.pop(("learned", 2))


# ---- end to end --------------------------------------------------------------------------------------------------------------
def _problem(seed, learned):
    """A seeded toy BOCF problem (m = 2 attributes of a smooth simulator on [0, 1]^2), built in the same order every time."""
    np.random.seed(seed)
    d, m = 2, 2
    space = B.Design_space([{'name': 'x', 'type': 'continuous', 'domain': (0, 1), 'dimensionality': d}])
    f = [lambda x: np.sin(3 * x[:, :1]) * x[:, 1:2] + x[:, :1] ** 2, lambda x: np.cos(2 * x[:, 1:2]) + 0.5 * x[:, :1]]
    objective = B.MultiObjective(f, noise_var=[1e-4, 1e-4])
    if learned:
        model = B.multi_outputGP(m, exact_feval=[True] * m, fixed_hyps=False, n_samples=10)
        model.n_burnin, model.subsample_interval, model.leapfrog_steps = 20, 2, 5
        support = np.array([[2.5, -1.5], [-1.0, 2.5]])          # out of reach: utilities of order one
        U = B.Utility(func=lambda t, y: -np.sum(np.square((np.asarray(y).T - t).T), axis=0), dfunc=lambda t, y: -2 * (np.asarray(y) - t),
                      parameter_dist=B.ParameterDistribution(support=support, prob_dist=np.array([0.3, 0.7])))
        psi = B.ExpectationUtility(lambda t, mu, var: -np.sum(np.square((mu.T - t).T), axis=0) - np.sum(var, axis=0),
                                   lambda t, mu, var: -np.concatenate((2 * (np.squeeze(mu) - t), np.ones(len(np.squeeze(var))))))
    else:
        model = B.multi_outputGP(m, kernel=[B.kern.RBF(d, variance=1.0, lengthscale=0.3, ARD=True) for _ in range(m)], noise_var=[1e-4] * m,
                                 fixed_hyps=True)
        support = np.array([[0.0], [1.0]])
        c = C_EXPCOS[2]
        U = B.Utility(func=lambda t, y: -np.tensordot(c, np.exp(-np.asarray(y) / np.pi) * np.cos(np.pi * np.asarray(y)), axes=(0, 0)),
                      dfunc=lambda t, y: O.utility_grad("neg_exp_cos", t, y, c),
                      parameter_dist=B.ParameterDistribution(support=support, prob_dist=np.array([0.5, 0.5])))
        psi = None
    opt = B.AcquisitionOptimizer(space, optimizer='lbfgs', n_starting=400, n_anchor=16)
    acq = B.uEI_noiseless(model, space, optimizer=opt, utility=U)
    X0 = np.random.uniform(size=(6, d))
    return space, objective, model, acq, U, psi, X0


def _loop_here(seed, learned, iters=3):
    """cbo.py:274-330 written out with the same pieces; the recommendation by the host restatement (_restated) and
    lbfgsb_batched_numpy, one parameter at a time (GeneralOptimizer.optimize)."""
    space, objective, model, acq, U, psi, X = _problem(seed, learned)
    m, bounds = 2, space.get_bounds()
    kind = "neg_sq_dist" if learned else "neg_exp_cos"
    params = None if learned else C_EXPCOS[2]
    Y, _ = objective.evaluate(X)
    model.updateModel(X, Y)
    current, suggested = np.atleast_2d(X[0]), X
    out = dict(suggestions=[], argmaxes=[], values=[], anchors=[])
    n_h = min(10, model.number_of_hyps_samples())
    for it in range(iters):
        model.updateModel(X, Y)
        x, _ = acq.optimize(x_baseline=current)
        assert not np.all(x == suggested)
        suggested = x
        out["suggestions"].append(x.copy())
        X = np.vstack((X, x))
        Yn, _ = objective.evaluate_w_noise(x)
        for j in range(m):
            Y[j] = np.vstack((Y[j], Yn[j]))
        model.updateModel(X, list(Y))
        support, prob = U.parameter_dist.support, U.parameter_dist.prob_dist
        val, argmaxes, anchors = 0, [], []
        for l in range(len(support)):
            Z = np.random.normal(size=(50, m)) if psi is None else None
            design = np.zeros((200, 2))
            for k in range(2):
                design[:, k] = np.random.uniform(low=bounds[k][0], high=bounds[k][1], size=200)

            def ev(Xe, grad):
                return _restated(model, Xe, "closed" if psi else "mc", kind, support, np.full(len(np.atleast_2d(Xe)), l),
                                 None if Z is None else {l: Z}, n_h, params, grad)
            scores = -ev(design, False)[0]
            idx = np.argsort(scores, kind="stable")[:24]
            anc, avals = design[idx], scores[idx]
            anchors.append(anc)
            Xopt, _ = lbfgsb_batched_numpy(lambda Xe: tuple(-a for a in ev(Xe, True)), anc, bounds, maxiter=500, factr=1e6)
            fx = -ev(Xopt, False)[0]
            b = int(np.argmin(fx))
            xl = Xopt[b] if not avals[0] < fx[b] else anc[0]
            argmaxes.append(xl)
            yv = np.reshape(objective.evaluate(np.atleast_2d(xl))[0], (m,))
            val += U.eval_func(support[l], yv) * prob[l]
        current = np.atleast_2d(argmaxes[-1])
        out["argmaxes"].append(np.array(argmaxes))
        out["values"].append(float(np.squeeze(val)))
        out["anchors"].append(np.array(anchors))
    return out


class _RecordingSequential(B.Sequential):
    def __init__(self, acquisition):
        super(_RecordingSequential, self).__init__(acquisition)
        self.seen = []

    def compute_batch(self, duplicate_manager=None, context_manager=None, x_baseline=None):
        x = super(_RecordingSequential, self).compute_batch(duplicate_manager, context_manager, x_baseline)
        self.seen.append(x.copy())
        return x


@pytest.mark.parametrize("learned", [False, True])
def test_cbo_run_optimization_matches_the_loop_written_out(learned, tmp_path):
    seed = 31 if learned else 17
    space, objective, model, acq, U, psi, X0 = _problem(seed, learned)
    ev = _RecordingSequential(acq)
    bo = B.CBO(model, space, objective, acq, ev, X0, expectation_utility=psi)
    recs, anchors = [], []
    orig = bo._recommend

    def rec(parameters):
        x = orig(parameters)
        recs.append(x.copy())
        anchors.append(bo.last_recommendation["anchors"].copy())
        return x
    bo._recommend = rec
    path = str(tmp_path / "results.txt")
    bo.run_optimization(max_iter=3, results_file=path)
    want = _loop_here(seed, learned)
    np.testing.assert_array_equal(ev.seen[0], want["suggestions"][0])
    for it in range(1, 3):
        np.testing.assert_allclose(ev.seen[it], want["suggestions"][it], rtol=0, atol=1e-4)
    np.testing.assert_array_equal(anchors[0], want["anchors"][0])
    for it in range(3):
        np.testing.assert_allclose(recs[it], want["argmaxes"][it], rtol=0, atol=1e-4)
    np.testing.assert_allclose(bo.historical_optimal_values, want["values"], rtol=1e-6)
    np.testing.assert_array_equal(bo.current_argmax, np.atleast_2d(recs[-1][-1]))
    res = np.loadtxt(path)
    assert res.shape == (3, 2) and np.all(np.diff(res[:, 1]) > 0)
    np.testing.assert_allclose(res[:, 0], bo.historical_optimal_values, rtol=1e-15)
