"""Joint posterior covariance, joint posterior samples and composite Thompson selection on the device against NumPy restatements of
posterior.py:104-125 built from the oracle's factors; CompositeThompsonBatch driving CBO end to end."""

import numpy as np
import pytest
from scipy.linalg import cholesky, solve_triangular

import bocf_amd as B
from bocf_amd import _ffi
from oracle import cpu_ref as R

pytestmark = pytest.mark.gpu

KINDS = {"rbf": B.kern.RBF, "se": B.kern.SE, "matern52": B.kern.Matern52, "matern32": B.kern.Matern32}

def _setup(kinds, N, d, seed, ls=0.4, noise=1e-2):
    rng = np.random.RandomState(seed)
    m = len(kinds)
    X = rng.uniform(size=(N, d))
    Y = [np.sin(3 * X[:, :1] + j) + 0.3 * X[:, 1:2] * (j + 1) for j in range(m)]
    var = 0.5 + rng.uniform(size=m)
    lss = [ls * (0.8 + 0.4 * rng.uniform(size=d)) for _ in range(m)]
    model = B.multi_outputGP(m, kernel=[KINDS[kinds[j]](d, variance=var[j], lengthscale=lss[j], ARD=True) for j in range(m)],
                             noise_var=[noise] * m, fixed_hyps=True)
    model.updateModel(X, Y)
    ref = R.MultiOutputGPRef(list(kinds), var, lss, [noise] * m)
    ref.updateModel(X, Y)
    return model, ref, var

def _ref_cov(ref, X1, X2):
    out = []
    for o in ref.output:
        A1 = solve_triangular(o.L, R.kern_K(o.kind, o.X, X1, o.variance, o.lengthscale), lower=True)
        A2 = solve_triangular(o.L, R.kern_K(o.kind, o.X, X2, o.variance, o.lengthscale), lower=True)
        out.append(R.kern_K(o.kind, X1, X2, o.variance, o.lengthscale) - A1.T.dot(A2))
    return np.stack(out)

@pytest.mark.parametrize("kinds", [("rbf",), ("se",), ("matern52",), ("matern32",), ("rbf", "matern32", "se"), ("matern52", "matern52", "rbf")])
@pytest.mark.parametrize("n", [1, 127, 128, 129, 300])
def test_posterior_covariance_against_the_oracle(kinds, n):
    d = 3
    model, ref, var = _setup(kinds, 200, d, 11 + n)
    rng = np.random.RandomState(n)
    X1, X2 = rng.uniform(size=(n, d)), rng.uniform(size=(n + 5, d))
    tol = 1e-10 * var.max()
    cov = model.posterior_covariance_between_points(X1, X2)
    assert cov.shape == (len(kinds), n, n + 5)
    np.testing.assert_allclose(cov, _ref_cov(ref, X1, X2), rtol=0, atol=tol)
    sym = model.posterior_covariance_between_points(X1, X1)
    np.testing.assert_allclose(sym, _ref_cov(ref, X1, X1), rtol=0, atol=tol)
    diag = np.einsum("jii->ji", sym)
    v = model.posterior_variance_noiseless(X1)
    keep = v > 1e-10
    np.testing.assert_allclose(diag[keep], v[keep], rtol=0, atol=tol)

def _sample_check(model, ref, Xc, S, seed):
    m = model.output_dim
    Z = np.random.RandomState(seed).normal(size=(m, Xc.shape[0], S))
    F = model.posterior_samples_f(Xc, size=S, Z=Z)
    jit = model.last_sample_jitter
    Sig = _ref_cov(ref, Xc, Xc)
    mu = ref.posterior_mean(Xc)
    return F, Z, jit, Sig, mu

@pytest.mark.parametrize("kinds", [("rbf", "matern52"), ("matern32", "se")])
@pytest.mark.parametrize("C", [127, 129])
@pytest.mark.parametrize("S", [1, 7, 64])
def test_samples_well_conditioned(kinds, C, S):
    model, ref, var = _setup(kinds, 150, 2, 5, ls=0.05)
    Xc = np.random.RandomState(C + S).uniform(size=(C, 2))
    F, Z, jit, Sig, mu = _sample_check(model, ref, Xc, S, C * S)
    assert F.shape == (2, C, S)
    for j in range(2):
        rung0 = 1e-8 * max(np.mean(np.diag(Sig[j])), 1e-10)
        np.testing.assert_allclose(jit[j], rung0, rtol=1e-8)
        L = cholesky(Sig[j] + jit[j] * np.eye(C), lower=True)
        np.testing.assert_allclose(F[j], mu[j][:, None] + L.dot(Z[j]), rtol=0, atol=1e-8 * var.max())

def test_samples_ill_conditioned_engage_the_ladder():
    """2048 candidates in a 0.02-wide box of a model with noise 1e-6: the posterior covariance is numerically rank-deficient, rung 0
    (1e-8 mean(diag)) does not factor it and the ladder climbs -- to the rung the same ladder needs on the oracle's covariance, give or
    take one (a reordered contraction alone moves it by one on the CPU).  The samples agree with mu + L_oracle Z in a measure that
    cond(L) does not amplify, ||F - mu - L Z|| / (||L||_2 ||Z||) <= 1e-4 (2.6e-6 for the reordered contraction on the CPU); whitening
    with the oracle's factor recovers Z to a relative error bounded by 1e-6 mean(diag) / jitter."""
    model, ref, var = _setup(("rbf", "matern52"), 512, 2, 9, ls=0.5, noise=1e-6)
    Xc = 0.3 + 0.02 * np.random.RandomState(1).uniform(size=(2048, 2))
    F, Z, jit, Sig, mu = _sample_check(model, ref, Xc, 4, 2)
    rung0 = np.array([1e-8 * max(np.mean(np.diag(Sig[j])), 1e-10) for j in range(2)])
    assert np.any(jit > rung0 * 1.5), (jit, rung0)
    for j in range(2):
        C = Xc.shape[0]
        r_dev = int(round(np.log10(jit[j] / rung0[j])))
        r_ref = 0
        while True:
            try:
                cholesky(Sig[j] + rung0[j] * 10.0 ** r_ref * np.eye(C), lower=True)
                break
            except np.linalg.LinAlgError:
                r_ref += 1
        assert abs(r_dev - r_ref) <= 1, (j, r_dev, r_ref)
        L = cholesky(Sig[j] + jit[j] * np.eye(C), lower=True)
        res = np.linalg.norm(F[j] - mu[j][:, None] - L.dot(Z[j])) / (np.linalg.norm(L, 2) * np.linalg.norm(Z[j]))
        assert res <= 1e-4, (j, res)
        Zr = solve_triangular(L, F[j] - mu[j][:, None], lower=True)
        err = np.linalg.norm(Zr - Z[j]) / np.linalg.norm(Z[j])
        assert err <= 1e-6 * np.mean(np.diag(Sig[j])) / jit[j], (j, err, np.mean(np.diag(Sig[j])) / jit[j])


def _raw_fit(ctx, X, Y, H, var, ls, noise):
    lib = _ffi.load()
    N, d = X.shape
    M = Y.shape[0]
    ctx.set_option("hyper_samples", H)
    _ffi.check(lib.bocf_fit(ctx.handle, _ffi.dptr(_ffi.f64(X)), _ffi.dptr(_ffi.f64(Y)), N, d, M, _ffi.KERN_RBF, _ffi.dptr(_ffi.f64(var)),
                            _ffi.dptr(_ffi.f64(ls)), _ffi.dptr(_ffi.f64(noise)), 5, None, None), "bocf_fit")

def test_hyper_sample_groups():
    rng = np.random.RandomState(4)
    N, d, m, H, C, S = 100, 2, 2, 3, 140, 5
    X = rng.uniform(size=(N, d))
    Y = rng.normal(size=(H * m, N))
    var = 0.5 + rng.uniform(size=H * m)
    ls = 0.2 + 0.3 * rng.uniform(size=(H * m, d))
    ctx = _ffi.Context(0)
    lib = _ffi.load()
    _raw_fit(ctx, X, Y, H, var, ls, np.full(H * m, 1e-2))
    Xc = rng.uniform(size=(C, d))
    _ffi.check(lib.bocf_set_candidates(ctx.handle, _ffi.dptr(_ffi.f64(Xc)), C), "bocf_set_candidates")
    Z = rng.normal(size=(H * m, C, S))
    F_all, j_all = np.empty_like(Z), np.empty(H * m)
    assert lib.bocf_posterior_samples(ctx.handle, -1, _ffi.dptr(Z), S, 10, _ffi.dptr(F_all), _ffi.dptr(j_all)) == 0
    for h in range(H):
        Zh = np.ascontiguousarray(Z[h * m:(h + 1) * m])
        F, jit = np.empty_like(Zh), np.empty(m)
        assert lib.bocf_posterior_samples(ctx.handle, h, _ffi.dptr(Zh), S, 10, _ffi.dptr(F), _ffi.dptr(jit)) == 0
        np.testing.assert_array_equal(F, F_all[h * m:(h + 1) * m])
        np.testing.assert_array_equal(jit, j_all[h * m:(h + 1) * m])
        cov = np.empty((m, 7, C))
        _ffi.check(lib.bocf_posterior_cov(ctx.handle, _ffi.dptr(_ffi.f64(Xc[:7])), 7, _ffi.dptr(_ffi.f64(Xc)), C, h, _ffi.dptr(cov)), "cov")
        allc = np.empty((H * m, 7, C))
        _ffi.check(lib.bocf_posterior_cov(ctx.handle, _ffi.dptr(_ffi.f64(Xc[:7])), 7, _ffi.dptr(_ffi.f64(Xc)), C, -1, _ffi.dptr(allc)), "cov")
        np.testing.assert_array_equal(cov, allc[h * m:(h + 1) * m])

NAMES = {_ffi.KERN_RBF: "rbf", _ffi.KERN_SE: "se", _ffi.KERN_MATERN52: "matern52", _ffi.KERN_MATERN32: "matern32"}


def _learned(H=4, N=40, m=2, d=2, seed=12):
    """A model with learned hyper-parameters (optimiser + HMC through updateModel): H hyper-samples resident on the device."""
    rng = np.random.RandomState(seed)
    X = rng.uniform(size=(N, d))
    Y = [np.sin(3 * X[:, :1] + j) + 0.1 * rng.normal(size=(N, 1)) for j in range(m)]
    np.random.seed(seed)
    model = B.multi_outputGP(m, fixed_hyps=False, n_samples=H)
    model.n_burnin, model.subsample_interval, model.leapfrog_steps = 20, 2, 5
    model.updateModel(X, Y)
    assert model._H == H
    return model, X, Y


def test_hyper_samples_of_a_learned_model():
    """set_hyperparameters(h) + posterior_samples_f / posterior_covariance_between_points answer for hyper-sample h: the device call
    with group = h, and the oracle built from that sample's hyper-parameters."""
    H, m, C, S = 4, 2, 130, 5
    model, X, Y = _learned(H=H, m=m)
    lib = _ffi.load()
    kids, var, ls, noise = model._hyper_arrays()
    Xc = np.random.RandomState(5).uniform(size=(C, 2))
    Z = np.random.RandomState(6).normal(size=(m, C, S))
    Fs = []
    for h in range(H):
        model.set_hyperparameters(h)
        F = model.posterior_samples_f(Xc, Z=Z)
        jit = model.last_sample_jitter.copy()
        Fd, jd = np.empty_like(F), np.empty(m)
        assert lib.bocf_posterior_samples(model._context().handle, h, _ffi.dptr(_ffi.f64(Z)), S, model.sample_jitter_tries, _ffi.dptr(Fd),
                                          _ffi.dptr(jd)) == 0
        np.testing.assert_array_equal(F, Fd)
        np.testing.assert_array_equal(jit, jd)
        r = slice(h * m, (h + 1) * m)
        ref = R.MultiOutputGPRef([NAMES[k] for k in kids[r]], var[r], list(ls[r]), noise[r])
        ref.updateModel(X, Y)
        model.set_hyperparameters(h)
        cov = model.posterior_covariance_between_points(Xc[:20], Xc)
        np.testing.assert_allclose(cov, _ref_cov(ref, Xc[:20], Xc), rtol=0, atol=1e-9 * var[r].max())
        Sig = _ref_cov(ref, Xc, Xc)
        for j in range(m):
            L = cholesky(Sig[j] + jit[j] * np.eye(C), lower=True)
            np.testing.assert_allclose(F[j], ref.posterior_mean(Xc)[j][:, None] + L.dot(Z[j]), rtol=0, atol=1e-7 * var[r].max())
        Fs.append(F)
    assert not np.array_equal(Fs[0], Fs[1])                 # the hyper-samples differ: group h is not group 0


def test_thompson_topk_mixes_hyper_samples():
    """thompson_topk with paths of several hyper-samples, out of order: one sampling call per hyper-sample, theta reordered to the
    device's path order and the results scattered back.  Path s against a NumPy top-k of U(theta_s, .) over that path's samples."""
    H, m, C, k = 4, 2, 200, 6
    model, X, Y = _learned(H=H, m=m, seed=13)
    groups = np.array([2, 0, 3, 1, 0, 2, 3, 2])
    P = groups.size
    rng = np.random.RandomState(7)
    Xc = rng.uniform(size=(C, 2))
    thetas = rng.normal(size=(P, m))
    Z = {h: rng.normal(size=(m, C, int(np.sum(groups == h)))) for h in range(H)}
    U = B.Utility(parameter_dist=B.ParameterDistribution(support=thetas, prob_dist=np.full(P, 1.0 / P)), device="neg_sq_dist")
    idx, val = model.thompson_topk(Xc, thetas, groups, Z, U, k)
    assert idx.shape == (P, k) and val.shape == (P, k)
    for h in range(H):
        model.set_hyperparameters(h)
        F = model.posterior_samples_f(Xc, Z=Z[h])
        for col, s in enumerate(np.flatnonzero(groups == h)):
            u = R.utility_eval("neg_sq_dist", thetas[s], F[:, :, col])
            order = np.lexsort((np.arange(C), -u))[:k]
            np.testing.assert_array_equal(idx[s], order)
            np.testing.assert_allclose(val[s], u[order], rtol=1e-13, atol=1e-13)


UTILS = [("linear", _ffi.UTIL_LINEAR, None), ("neg_sq_dist", _ffi.UTIL_NEG_SQ_DIST, None), ("neg_sum_exp", _ffi.UTIL_NEG_SUM_EXP, None),
         ("neg_exp_cos", _ffi.UTIL_NEG_EXP_COS, np.array([1.0, 0.5, 2.0])), ("rosenbrock", _ffi.UTIL_ROSENBROCK, None)]

@pytest.mark.parametrize("name,kind,params", UTILS)
def test_thompson_select_against_numpy(name, kind, params):
    model, ref, var = _setup(("rbf", "matern32", "se"), 120, 2, 8)
    C, S, k = 300, 6, 9
    Xc = np.random.RandomState(6).uniform(size=(C, 2))
    Z = np.random.RandomState(7).normal(size=(3, C, S))
    F = model.posterior_samples_f(Xc, Z=Z)
    th = np.random.RandomState(8).normal(size=(S, 3))
    if name == "linear":
        th[2] = 0.0                                             # every candidate ties: indices 0 .. k - 1
    lib = _ffi.load()
    idx, val = np.empty((S, k), dtype=np.int64), np.empty((S, k))
    pa = None if params is None else _ffi.f64(params)
    _ffi.check(lib.bocf_thompson_select(model._context().handle, kind, _ffi.dptr(pa), 0 if pa is None else pa.size, _ffi.dptr(_ffi.f64(th)), 3, k,
                                        idx.ctypes.data_as(_ffi._c_ll_p), _ffi.dptr(val)), "bocf_thompson_select")
    for s in range(S):
        u = R.utility_eval(name, th[s], F[:, :, s], params)
        order = np.lexsort((np.arange(C), -u))[:k]
        np.testing.assert_array_equal(idx[s], order)
        np.testing.assert_allclose(val[s], u[order], rtol=1e-13, atol=1e-13)
    if name == "linear":
        np.testing.assert_array_equal(idx[2], np.arange(k))

def test_errors_leave_the_context_usable():
    lib = _ffi.load()
    fresh = _ffi.Context(0)
    out = np.empty((1, 1, 1))
    x = np.zeros((1, 2))
    assert lib.bocf_posterior_cov(fresh.handle, _ffi.dptr(x), 1, _ffi.dptr(x), 1, -1, _ffi.dptr(out)) < 0
    assert b"not fitted" in lib.bocf_last_error()
    model, ref, var = _setup(("rbf",), 60, 2, 1)
    h = model._context().handle
    Xc = np.random.RandomState(0).uniform(size=(1024, 2))
    idx, val = np.empty((1, 2), dtype=np.int64), np.empty((1, 2))
    th = np.zeros((1, 1))
    model._set_candidates(Xc)
    assert lib.bocf_thompson_select(h, 0, None, 0, _ffi.dptr(th), 1, 2, idx.ctypes.data_as(_ffi._c_ll_p), _ffi.dptr(val)) < 0
    assert b"no resident samples" in lib.bocf_last_error()
    Z = np.zeros((1, 1024, 2))
    assert lib.bocf_posterior_samples(h, -1, _ffi.dptr(Z), 0, 5, None, None) < 0
    assert lib.bocf_posterior_samples(h, -1, _ffi.dptr(Z), 257, 5, None, None) < 0
    model.set_option("workspace_mb", 4)                     # 1024^2 x 8 B = 8 MiB
    assert lib.bocf_posterior_samples(h, -1, _ffi.dptr(Z), 2, 5, None, None) < 0
    assert b"workspace_mb" in lib.bocf_last_error()
    np.testing.assert_allclose(model.predict(Xc[:5])[0], ref.predict(Xc[:5])[0], rtol=1e-6, atol=1e-8)
    model.set_option("workspace_mb", 24576)
    model._set_candidates(Xc[:10])
    assert lib.bocf_posterior_samples(h, -1, _ffi.dptr(np.zeros((1, 10, 2))), 2, 5, None, None) == 0
    assert lib.bocf_thompson_select(h, 0, None, 0, _ffi.dptr(th), 1, 11, idx.ctypes.data_as(_ffi._c_ll_p), None) < 0      # k > C
    assert lib.bocf_posterior_samples(h, 3, _ffi.dptr(np.zeros((1, 10, 2))), 2, 5, None, None) < 0                      # no such group
    # a host-given posterior has no factor
    canned = _ffi.Context(0)
    mean, vv, mt = np.zeros((1, 4)), np.ones((1, 4)), np.zeros((1, 3))
    _ffi.check(lib.bocf_set_posterior(canned.handle, 1, 4, 3, _ffi.dptr(mean), _ffi.dptr(vv), _ffi.dptr(mt)), "bocf_set_posterior")
    assert lib.bocf_posterior_samples(canned.handle, -1, _ffi.dptr(np.zeros((1, 4, 1))), 1, 5, None, None) < 0
    assert b"host-given posterior" in lib.bocf_last_error()
    np.testing.assert_allclose(model.predict(Xc[:5])[1], ref.predict(Xc[:5])[1], rtol=1e-6, atol=1e-8)

def _cbo_problem(seed, q, evaluator_cls=None):
    np.random.seed(seed)
    d, m = 2, 2
    space = B.Design_space([{'name': 'x', 'type': 'continuous', 'domain': (0, 1), 'dimensionality': d}])
    f = [lambda x: np.sin(3 * x[:, :1]) * x[:, 1:2] + x[:, :1] ** 2, lambda x: np.cos(2 * x[:, 1:2]) + 0.5 * x[:, :1]]
    objective = B.MultiObjective(f, noise_var=[1e-4, 1e-4])
    model = B.multi_outputGP(m, kernel=[B.kern.RBF(d, variance=1.0, lengthscale=0.3, ARD=True) for _ in range(m)], noise_var=[1e-4] * m,
                             fixed_hyps=True)
    U = B.Utility(parameter_dist=B.ParameterDistribution(support=np.array([[0.5, 0.2], [0.1, 0.9]]), prob_dist=np.array([0.5, 0.5])),
                  device="neg_sq_dist")
    opt = B.AcquisitionOptimizer(space, optimizer='lbfgs', n_starting=100, n_anchor=4)
    acq = B.uEI_noiseless(model, space, optimizer=opt, utility=U)
    X0 = np.random.uniform(size=(5, d))
    ev = evaluator_cls(acq) if evaluator_cls else B.CompositeThompsonBatch(acq, q, n_candidates=1024)
    return B.CBO(model, space, objective, acq, ev, X0)

def test_cbo_with_composite_thompson_batches():
    bo = _cbo_problem(21, 4)
    bo.run_optimization(max_iter=3)
    assert bo.X.shape == (5 + 3 * 4, 2)
    assert np.all(bo.X >= 0.0) and np.all(bo.X <= 1.0)
    for it in range(3):
        rows = bo.X[5 + 4 * it:5 + 4 * (it + 1)]
        assert len({tuple(r) for r in rows}) == 4
    assert [y.shape for y in bo.Y] == [(17, 1), (17, 1)]

def test_cbo_batch_of_one_is_sequential():
    a = _cbo_problem(22, 1)
    a.run_optimization(max_iter=2)
    b = _cbo_problem(22, 1, evaluator_cls=B.Sequential)
    b.run_optimization(max_iter=2)
    np.testing.assert_array_equal(a.X, b.X)
    np.testing.assert_array_equal(a.historical_optimal_values, b.historical_optimal_values)


def test_cbo_with_composite_thompson_batches_learned():
    np.random.seed(23)
    d, m, q = 2, 2, 6
    space = B.Design_space([{'name': 'x', 'type': 'continuous', 'domain': (0, 1), 'dimensionality': d}])
    f = [lambda x: np.sin(3 * x[:, :1]) * x[:, 1:2] + x[:, :1] ** 2, lambda x: np.cos(2 * x[:, 1:2]) + 0.5 * x[:, :1]]
    objective = B.MultiObjective(f, noise_var=[1e-4, 1e-4])
    model = B.multi_outputGP(m, exact_feval=[True] * m, fixed_hyps=False, n_samples=3)
    model.n_burnin, model.subsample_interval, model.leapfrog_steps = 20, 2, 5
    U = B.Utility(parameter_dist=B.ParameterDistribution(support=np.array([[0.5, 0.2], [0.1, 0.9]]), prob_dist=np.array([0.5, 0.5])),
                  device="neg_sq_dist")
    acq = B.uEI_noiseless(model, space, optimizer=B.AcquisitionOptimizer(space, optimizer='lbfgs', n_starting=100, n_anchor=4), utility=U)
    X0 = np.random.uniform(size=(6, d))
    bo = B.CBO(model, space, objective, acq, B.CompositeThompsonBatch(acq, q, n_candidates=512), X0)
    bo.run_optimization(max_iter=2)
    assert bo.X.shape == (6 + 2 * q, 2)
    assert np.all(bo.X >= 0.0) and np.all(bo.X <= 1.0)
    for it in range(2):
        assert len({tuple(r) for r in bo.X[6 + q * it:6 + q * (it + 1)]}) == q
