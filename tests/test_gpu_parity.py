"""GPU parity: the HIP path (through the Python plug-in classes -> ctypes -> C ABI) against the
golden vectors produced by the reference's own code and against the oracle on seeded inputs.
Run on the MI355X box:  python -m pytest tests -m gpu"""
import numpy as np
import pytest

from oracle import cpu_ref as R

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def B():
    import bocf_amd
    bocf_amd._ffi.load()          # fail loudly if the HIP library is missing
    return bocf_amd


def _kern(B, kind, d, var, ls):
    cls = {"rbf": B.kern.RBF, "se": B.kern.SE, "matern52": B.kern.Matern52, "matern32": B.kern.Matern32}[kind]
    ls = np.atleast_1d(ls)
    return cls(d, variance=var, lengthscale=ls, ARD=ls.size > 1)


def _model(B, kind, X, Ys, variances, lengthscales, noises):
    d = X.shape[1]
    m = len(Ys)
    model = B.multi_outputGP(m, kernel=[_kern(B, kind, d, variances[j], lengthscales[j]) for j in range(m)],
                             noise_var=list(noises), fixed_hyps=True)
    model.updateModel(X, Ys)
    return model


# ---------------------------------------------------------------------------------------------
# row A: kernel build vs the reference's K(X) (golden)
@pytest.mark.parametrize("kind", ["rbf", "se", "matern52", "matern32"])
@pytest.mark.parametrize("ard", ["ard", "iso"])
def test_train_kernel_golden(B, golden, kind, ard):
    g = golden("kernels")
    t = "%s_%s_N40" % (kind, ard)
    X = g[t + "_X"]
    model = _model(B, kind, X, [np.sin(X.sum(1))[:, None]], [float(g[t + "_var"])], [g[t + "_ls"]], [1e-6])
    K = model.get_train_kernel(0)
    np.testing.assert_allclose(K, g[t + "_K"], rtol=1e-12, atol=1e-14)
    np.testing.assert_array_equal(K, K.T)


# rows B, C, D, E: factor, alpha, log-marginal, raw predictive mean/variance (golden)
@pytest.mark.parametrize("tag,kind", [("se_N64", "se"), ("se_N64_noisy", "se"), ("rbf_N96", "rbf"), ("m52_N96", "matern52")])
def test_fit_predict_golden(B, golden, tag, kind):
    g = golden("fit_predict")
    X, Y, Xs = g[tag + "_X"], g[tag + "_Y"], g[tag + "_Xs"]
    noise, var = float(g[tag + "_noise"]), float(g[tag + "_var"])
    model = _model(B, kind, X, [Y], [var], [g[tag + "_ls"]], [noise])
    assert model.jitter[0] == 0.0
    L, alpha = model.get_factor(0)
    np.testing.assert_allclose(L, g[tag + "_L"], rtol=1e-6, atol=1e-9)
    scale = np.abs(g[tag + "_alpha"]).max()
    np.testing.assert_allclose(alpha[:, None], g[tag + "_alpha"], rtol=1e-5, atol=1e-7 * scale)
    np.testing.assert_allclose(model.log_marginal[0], g[tag + "_lml"], rtol=1e-9)
    ymean = Y.mean()
    mu = model.posterior_mean(Xs)
    np.testing.assert_allclose(mu[0], g[tag + "_raw_mean"][:, 0] + ymean, rtol=1e-5, atol=1e-6)
    v = model.posterior_variance_noiseless(Xs)
    ref = np.clip(g[tag + "_raw_var"][:, 0], 1e-10, np.inf)
    assert np.abs(v[0] - ref).max() <= 1e-5 * var * 1e-3 + 1e-10     # 1e-8 sigma_f^2: far inside the 1e-5 gate
    mean2, v2 = model.predict(Xs)
    np.testing.assert_allclose(mean2, mu, rtol=0, atol=0)
    np.testing.assert_allclose(v2[0], np.clip(g[tag + "_raw_var"][:, 0] + noise, 1e-10, np.inf), rtol=1e-5, atol=1e-8 * var)
    np.testing.assert_allclose(model.posterior_variance(Xs), v2, rtol=0, atol=0)
    mu_tr = model.posterior_mean_at_evaluated_points()
    np.testing.assert_allclose(mu_tr[0], R.GPFit(kind, X, Y, var, g[tag + "_ls"], noise).posterior_mean(X)[:, 0], rtol=1e-5, atol=1e-6)


# jitchol ladder (GPy/util/linalg.py:52-71) through the diag-shift test hook, against the oracle
def test_jitter_ladder(B, probes):
    rng = np.random.RandomState(7)
    N, d = 200, 2
    X = rng.uniform(size=(N, d))
    Y = np.sin(3 * X.sum(1))[:, None]
    var, ls, noise = 1.0, np.array([0.9]), 1e-6
    K = R.kern_K("se", X, None, var, ls)
    lam = np.linalg.eigvalsh(K)
    model = B.multi_outputGP(1, kernel=[_kern(B, "se", d, var, ls)], noise_var=[noise], fixed_hyps=True)
    # make Ky indefinite by ~3e-4 so that jitter 1e-6, 1e-5, 1e-4 fail and 1e-3 succeeds
    shift = noise + 1e-8 + max(lam.min(), 0.0) + 3e-4
    model.set_option("test_diag_shift_1e12", int(round(shift * 1e12)))
    model.updateModel(X, [Y])
    Ky = K + (noise + 1e-8 - shift) * np.eye(N)
    Lref, jref = R.jitchol(Ky)
    assert jref > 0
    assert model.jitter[0] == pytest.approx(jref, rel=1e-12)
    L, _ = model.get_factor(0)
    np.testing.assert_allclose(L.dot(L.T), Ky + jref * np.eye(N), rtol=0, atol=1e-10)
    # hopeless case -> LinAlgError, as jitchol raises
    model2 = B.multi_outputGP(1, kernel=[_kern(B, "se", d, var, ls)], noise_var=[noise], fixed_hyps=True)
    model2.set_option("test_diag_shift_1e12", int(0.9e12))
    with pytest.raises(np.linalg.LinAlgError):
        model2.updateModel(X, [Y])


# rows F, G1, G2, H end to end vs the reference's acquisition classes (golden e2e)
@pytest.mark.parametrize("tag,kind,N,d,m,C,S", [("cfg1", "se", 64, 2, 1, 400, 25), ("cfg2s", "rbf", 128, 6, 4, 256, 32)])
def test_e2e_golden(B, golden, tag, kind, N, d, m, C, S):
    g = golden("e2e")
    p = R.synthetic_problem(N, d, m, C, S, int(g[tag + "_seed"]))
    model = _model(B, kind, p["X"], p["Y"], p["variances"], p["lengthscales"], p["noise"])
    np.testing.assert_allclose(model.log_marginal, g[tag + "_lml"], rtol=1e-8)
    mean, var = model.predict(p["Xc"])
    np.testing.assert_allclose(mean, g[tag + "_mean"], rtol=1e-5, atol=1e-6)
    assert np.abs(var - g[tag + "_var"]).max() <= 1e-5 * 1.0 * 1e-3 + 1e-10
    np.testing.assert_allclose(model.posterior_mean_at_evaluated_points(), g[tag + "_mu_eval"], rtol=1e-5, atol=1e-6)

    dist = B.ParameterDistribution(continuous=False, support=g[tag + "_theta"], prob_dist=np.ones(1))
    U = B.Utility(parameter_dist=dist, device="neg_sq_dist")
    np.random.seed(3)
    acq = B.uEI_noiseless(model, None, optimizer=None, utility=U)
    assert acq.W_samples.shape == (25, m)
    acq.W_samples = p["W"]
    a = acq._compute_acq(p["Xc"])
    assert a.shape == (C, 1)
    np.testing.assert_allclose(a, g[tag + "_uEI"], rtol=1e-5, atol=1e-12)
    np.testing.assert_array_equal(acq.acquisition_function(p["Xc"]), -a)
    sel = acq.select_anchors(16)
    _check_selection(a, sel, g[tag + "_sel_uEI"])

    upi = B.uPI(model, None, optimizer=None, utility=U)
    upi.W_samples = p["W"]
    np.testing.assert_allclose(upi._compute_acq(p["Xc"]), g[tag + "_uPI"], rtol=1e-5, atol=1e-12)

    dist_l = B.ParameterDistribution(continuous=False, support=g[tag + "_theta_lin"], prob_dist=np.ones(1))
    mae = B.maEI(model, None, optimizer=None, utility=B.Utility(parameter_dist=dist_l, linear=True))
    a = mae._compute_acq(p["Xc"])
    np.testing.assert_allclose(a, g[tag + "_maEI"], rtol=1e-5, atol=1e-12)
    _check_selection(a, mae.select_anchors(16), g[tag + "_sel_maEI"])


def _check_selection(acq, order, ref_order):
    acq = np.asarray(acq).flatten()
    np.testing.assert_allclose(acq[order], acq[ref_order], rtol=0, atol=0)
    for i, j in zip(order, ref_order):
        if np.sum(acq == acq[j]) == 1:
            assert i == j
    # ours: ties to the lowest index
    np.testing.assert_array_equal(order, np.argsort(-acq, kind="stable")[: len(order)])


# every device utility, L = 2 full support, both MC kinds, closed-form twins -- against the oracle
@pytest.mark.parametrize("util,m", [("neg_sq_dist", 3), ("neg_sum_exp", 3), ("neg_exp_cos", 3), ("rosenbrock", 4), ("linear", 3)])
def test_acquisitions_vs_oracle(B, util, m):
    N, d, C, S = 150, 3, 333, 50
    p = R.synthetic_problem(N, d, m, C, S, 99, noise=1e-4)
    model = _model(B, "matern52", p["X"], p["Y"], p["variances"], p["lengthscales"], p["noise"])
    ref = R.MultiOutputGPRef("matern52", p["variances"], p["lengthscales"], p["noise"])
    ref.updateModel(p["X"], p["Y"])
    rng = np.random.RandomState(5)
    params = None
    if util in ("neg_sq_dist", "linear"):
        support, prob = rng.normal(size=(2, m)) * 0.5, np.array([0.25, 0.75])
    elif util == "rosenbrock":
        support, prob = np.array([[1.0], [0.5]]), np.array([0.6, 0.4])
    else:
        support, prob = np.ones((1, 1)), np.ones(1)
        if util == "neg_exp_cos":
            params = np.array([1.0, 2.0, 5.0])
    U = B.Utility(parameter_dist=B.ParameterDistribution(support=support, prob_dist=prob), device=util, device_params=params)
    mu_eval = ref.posterior_mean_at_evaluated_points()
    mu, sig = ref.posterior_mean(p["Xc"]), np.sqrt(ref.posterior_variance(p["Xc"]))
    for cls, kind in ((B.uEI_noiseless, "EI"), (B.uPI, "PI")):
        acq = cls(model, None, utility=U)
        acq.W_samples = p["W"]
        a = acq._compute_acq(p["Xc"])
        r, _ = R.mc_acq(mu, sig, mu_eval, p["W"], util, support, prob, kind, util_params=params)
        if kind == "EI":
            np.testing.assert_allclose(a, r, rtol=1e-5, atol=1e-9)
        else:   # indicator sums may flip on a candidate whose utility sits within round-off of best
            assert np.mean(np.abs(a - r) > 1e-12) <= 0.01
            assert np.abs(a - r).max() <= 1.0 / S + 1e-12
    if util == "linear":
        mean, var = ref.predict(p["Xc"])
        for cls, kind in ((B.maEI, "EI"), (B.maPI, "PI")):
            a = cls(model, None, utility=U)._compute_acq(p["Xc"])
            r, _ = R.ma_acq(mean, var, mu_eval, support, prob, kind)
            np.testing.assert_allclose(a, r, rtol=1e-5, atol=1e-9)


def test_sampled_theta_rng_parity(B):
    """Not-full-support path: maEI draws 3 thetas per call with np.random.choice
    (maEI.py:46, parameter_distribution.py:27); same seed -> same draw as the oracle's replay."""
    m, N, d, C = 2, 100, 2, 64
    p = R.synthetic_problem(N, d, m, C, 8, 12, noise=1e-4)
    model = _model(B, "rbf", p["X"], p["Y"], p["variances"], p["lengthscales"], p["noise"])
    rng = np.random.RandomState(1)
    support, prob = rng.uniform(0.1, 1.0, size=(24, m)), np.full(24, 1.0 / 24)
    U = B.Utility(parameter_dist=B.ParameterDistribution(support=support, prob_dist=prob), linear=True)
    acq = B.maEI(model, None, utility=U)
    assert not acq.use_full_support
    np.random.seed(77)
    a = acq._compute_acq(p["Xc"])
    np.random.seed(77)
    idx = np.random.choice(24, size=3, p=prob)
    ref = R.MultiOutputGPRef("rbf", p["variances"], p["lengthscales"], p["noise"])
    ref.updateModel(p["X"], p["Y"])
    mean, var = ref.predict(p["Xc"])
    r, _ = R.ma_acq(mean, var, ref.posterior_mean_at_evaluated_points(), support[idx], None, "EI")
    np.testing.assert_allclose(a, r, rtol=1e-5, atol=1e-9)


# edge cases: empty / single / ragged batches, N not a multiple of the tile, chunked evaluation
def test_ragged_and_chunked(B):
    m, N, d = 2, 130, 4
    p = R.synthetic_problem(N, d, m, 1000, 16, 21, noise=1e-4)
    model = _model(B, "rbf", p["X"], p["Y"], p["variances"], p["lengthscales"], p["noise"])
    ref = R.MultiOutputGPRef("rbf", p["variances"], p["lengthscales"], p["noise"])
    ref.updateModel(p["X"], p["Y"])
    mean_full, var_full = model.predict(p["Xc"])
    rm, rv = ref.predict(p["Xc"])
    np.testing.assert_allclose(mean_full, rm, rtol=1e-5, atol=1e-6)
    assert np.abs(var_full - rv).max() <= 1e-8
    for n in (17, 127, 128, 129, 257):              # tile path: a candidate's numbers never depend on its batch
        mean, var = model.predict(p["Xc"][:n])
        np.testing.assert_array_equal(mean, mean_full[:, :n])
        np.testing.assert_array_equal(var, var_full[:, :n])
    for n in (1, 2, 16):                             # <= 16 candidates take the GEMV-shaped path: same values to round-off
        mean, var = model.predict(p["Xc"][:n])
        np.testing.assert_array_equal(mean, mean_full[:, :n])
        np.testing.assert_allclose(var, var_full[:, :n], rtol=1e-7, atol=1e-13)
        model.set_option("small_path", 0)
        mean_t, var_t = model.predict(p["Xc"][:n])
        model.set_option("small_path", 1)
        np.testing.assert_array_equal(var_t, var_full[:, :n])
    mean1, var1 = model.predict(p["Xc"][5])          # 1-D input promoted (gpmodel.py:144)
    np.testing.assert_array_equal(mean1[:, 0], mean_full[:, 5])
    e_mean, e_var = model.predict(np.empty((0, d)))
    assert e_mean.shape == (m, 0) and e_var.shape == (m, 0)
    for opt, val in (("swizzle", 258), ("prefetch1", 1)):   # tiling / staging options never change a number
        model.set_option(opt, val)
        mean_o, var_o = model.predict(p["Xc"])
        np.testing.assert_array_equal(mean_o, mean_full)
        np.testing.assert_array_equal(var_o, var_full)
        model.set_option(opt, 0)
    model.set_option("chunk", 256)                   # 1000 candidates in 4 passes: identical numbers
    mean_c, var_c = model.predict(p["Xc"])
    np.testing.assert_array_equal(mean_c, mean_full)
    np.testing.assert_array_equal(var_c, var_full)


def test_pickle_drops_handle(B):
    import pickle
    p = R.synthetic_problem(64, 2, 1, 50, 8, 3, noise=1e-4)
    model = _model(B, "se", p["X"], p["Y"], p["variances"], p["lengthscales"], p["noise"])
    a = model.predict(p["Xc"])
    clone = pickle.loads(pickle.dumps(model))
    b = clone.predict(p["Xc"])
    np.testing.assert_array_equal(a[0], b[0])
    np.testing.assert_array_equal(a[1], b[1])


# size-independent properties at BASELINE config 2 (m=4 RBF, N=1024, d=6, S=256, C=8192)
def test_config2_properties(B):
    N, d, m, C, S = 1024, 6, 4, 8192, 256
    p = R.synthetic_problem(N, d, m, C, S, 1236)
    model = _model(B, "rbf", p["X"], p["Y"], p["variances"], p["lengthscales"], p["noise"])
    # (1) identities at the training inputs: the noiseless variance collapses to the noise floor and
    #     K alpha = y_c - (noise + 1e-8) alpha  =>  mu(X_i) = y_i - (noise + 1e-8) alpha_i
    v_tr = model.posterior_variance_noiseless(p["X"][:512])
    assert v_tr.max() < 5e-6 and v_tr.min() >= 1e-10
    mu_tr = model.posterior_mean_at_evaluated_points()
    Y = np.stack([y[:, 0] for y in p["Y"]])
    alpha = np.stack([model.get_factor(j)[1] for j in range(m)])
    resid = mu_tr - (Y - (p["noise"][0] + 1e-8) * alpha)
    assert np.abs(resid).max() < 1e-6 * max(1.0, np.abs(alpha).max() * 1e-6)
    # (2) oracle parity on a slice the CPU finishes in seconds
    ref = R.MultiOutputGPRef("rbf", p["variances"], p["lengthscales"], p["noise"])
    ref.updateModel(p["X"], p["Y"])
    sl = slice(0, 512)
    mean, var = model.predict(p["Xc"])
    rm, rv = ref.predict(p["Xc"][sl])
    np.testing.assert_allclose(mean[:, sl], rm, rtol=1e-5, atol=1e-5)
    assert np.abs(var[:, sl] - rv).max() <= 1e-5 * 1.0 + 1e-10
    rel = np.abs(var[:, sl] - rv) / rv
    print("config2 variance: max rel err %.3e (values %.2e..%.2e)" % (rel.max(), rv.min(), rv.max()))
    assert rel.max() < 1e-4
    # (3) acquisition: sharding invariance (bit-exact) and selection consistency
    theta = np.array([[0.2 * (j + 1) for j in range(m)]])
    U = B.Utility(parameter_dist=B.ParameterDistribution(support=theta, prob_dist=np.ones(1)), device="neg_sq_dist")
    acq = B.uEI_noiseless(model, None, utility=U)
    acq.W_samples = p["W"]
    a = acq._compute_acq(p["Xc"])
    top = acq.select_anchors(16)
    np.testing.assert_array_equal(top, np.argsort(-a[:, 0], kind="stable")[:16])
    halves = np.concatenate([acq._compute_acq(p["Xc"][: C // 2]), acq._compute_acq(p["Xc"][C // 2:])])
    np.testing.assert_array_equal(a, halves)
    assert a.min() >= 0.0
    r, _, _ = R.batch_uEI(ref, p["Xc"][sl], p["W"], "neg_sq_dist", theta, np.ones(1), "EI")
    np.testing.assert_allclose(a[sl], r, rtol=1e-5, atol=1e-10)


def test_errors_are_loud(B):
    model = B.multi_outputGP(1, fixed_hyps=True)
    with pytest.raises(RuntimeError):
        model.predict(np.zeros((3, 2)))
    with pytest.raises(RuntimeError):
        B.multi_outputGP(1, fixed_hyps=False).predict(np.zeros((3, 2)))          # learning mode: no updateModel yet
    with pytest.raises(NotImplementedError):
        B.Utility(func=lambda t, y: np.abs(y).sum(0), parameter_dist=B.ParameterDistribution(support=np.ones((1, 1)), prob_dist=np.ones(1))).device_kind()
    p = R.synthetic_problem(32, 2, 1, 10, 4, 3)
    model.updateModel(p["X"], p["Y"])               # default kernel SE(2, 0.3), noise 1e-10 (gpmodel_fixed_hyps.py:50,56)
    ref = R.MultiOutputGPRef("se", [2.0], [np.array([0.3])], [1e-10])
    ref.updateModel(p["X"], p["Y"])
    mean, var = model.predict(p["Xc"])
    rm, rv = ref.predict(p["Xc"])
    np.testing.assert_allclose(mean, rm, rtol=1e-6, atol=1e-7)
    assert np.abs(var - rv).max() < 1e-8
    with pytest.raises(ValueError):
        model.predict(np.zeros((3, 5)))


# block counts that are not powers of two exercise the incomplete merges of the recursive inverse
@pytest.mark.parametrize("N", [641, 700, 1300])
def test_odd_block_counts(B, N):
    d, m, C = 5, 2, 300
    p = R.synthetic_problem(N, d, m, C, 8, 50 + N, noise=1e-5)
    model = _model(B, "rbf", p["X"], p["Y"], p["variances"], p["lengthscales"], p["noise"])
    ref = R.MultiOutputGPRef("rbf", p["variances"], p["lengthscales"], p["noise"])
    ref.updateModel(p["X"], p["Y"])
    mean, var = model.predict(p["Xc"])
    rm, rv = ref.predict(p["Xc"])
    np.testing.assert_allclose(mean, rm, rtol=1e-5, atol=1e-5)
    assert np.abs(var - rv).max() <= 1e-8
    np.testing.assert_allclose(model.log_marginal, [o.log_marginal for o in ref.output], rtol=1e-8)
    L, alpha = model.get_factor(1)
    np.testing.assert_allclose(L, ref.output[1].L, rtol=1e-5, atol=1e-8)


# gradient rows against the reference's own numbers (golden) and finite differences
@pytest.mark.parametrize("tag,kind,N,d,m,n,S", [("se", "se", 60, 3, 2, 7, 6), ("rbf", "rbf", 60, 3, 2, 7, 6), ("m52", "matern52", 50, 4, 3, 5, 5)])
def test_gradients_golden(B, golden, tag, kind, N, d, m, n, S):
    g = golden("gradients")
    p = R.synthetic_problem(N, d, m, n, S, int(g[tag + "_seed"]), noise=float(g[tag + "_noise"]))
    model = _model(B, kind, p["X"], p["Y"], p["variances"], p["lengthscales"], p["noise"])
    Xc = p["Xc"]
    dmean, dvar = model.posterior_mean_gradient(Xc), model.posterior_variance_gradient(Xc)
    assert dmean.shape == (m, n, d) and dvar.shape == (m, n, d)
    np.testing.assert_allclose(dmean, g[tag + "_dmean"], rtol=1e-5, atol=1e-6)
    np.testing.assert_allclose(dvar, g[tag + "_dvar"], rtol=1e-5, atol=1e-8)
    np.testing.assert_allclose(model.output[1].posterior_mean_gradient(Xc), g[tag + "_dmean"][1], rtol=1e-5, atol=1e-6)
    dist = B.ParameterDistribution(support=g[tag + "_support"], prob_dist=g[tag + "_prob"])
    for cls, name in ((B.maEI, "maEI"), (B.maPI, "maPI")):
        acq = cls(model, None, utility=B.Utility(parameter_dist=dist, linear=True))
        assert acq.analytical_gradient_acq
        a, da = acq._compute_acq_withGradients(Xc)
        np.testing.assert_allclose(a, g["%s_%s_acq" % (tag, name)], rtol=1e-5, atol=1e-12)
        np.testing.assert_allclose(da, g["%s_%s_dacq" % (tag, name)], rtol=1e-4, atol=1e-9)
        fa, fda = acq.acquisition_function_withGradients(Xc)
        np.testing.assert_array_equal(fa, -a)
        np.testing.assert_array_equal(fda, -da)
    for uname in ("neg_sq_dist", "neg_sum_exp"):
        dd = dist if uname == "neg_sq_dist" else B.ParameterDistribution(support=np.ones((1, 1)), prob_dist=np.ones(1))
        acq = B.uEI_noiseless(model, None, utility=B.Utility(parameter_dist=dd, device=uname))
        acq.W_samples = p["W"]
        a, da = acq._compute_acq_withGradients(Xc)
        np.testing.assert_allclose(a, g["%s_uEI_%s_acq" % (tag, uname)], rtol=1e-5, atol=1e-12)
        np.testing.assert_allclose(da, g["%s_uEI_%s_dacq" % (tag, uname)], rtol=1e-4, atol=1e-9)


def test_gradients_finite_differences(B):
    N, d, m, n = 300, 5, 3, 9
    p = R.synthetic_problem(N, d, m, n, 16, 77, noise=1e-3)
    model = _model(B, "matern52", p["X"], p["Y"], p["variances"], p["lengthscales"], p["noise"])
    Xc = p["Xc"]
    dmean, dvar = model.posterior_mean_gradient(Xc), model.posterior_variance_gradient(Xc)
    h = 1e-6
    for q in range(d):
        Xp, Xm = Xc.copy(), Xc.copy()
        Xp[:, q] += h
        Xm[:, q] -= h
        np.testing.assert_allclose(dmean[:, :, q], (model.posterior_mean(Xp) - model.posterior_mean(Xm)) / (2 * h), rtol=1e-4, atol=1e-5)
        fdv = (model.posterior_variance_noiseless(Xp) - model.posterior_variance_noiseless(Xm)) / (2 * h)
        np.testing.assert_allclose(dvar[:, :, q], fdv, rtol=1e-3, atol=1e-5)
    # the same gradients through the tile path (n = 9 <= 16 used the GEMV-shaped path above)
    model.set_option("small_path", 0)
    dmean_t, dvar_t = model.posterior_mean_gradient(Xc), model.posterior_variance_gradient(Xc)
    model.set_option("small_path", 1)
    np.testing.assert_allclose(dmean_t, dmean, rtol=1e-12, atol=1e-14)
    np.testing.assert_allclose(dvar_t, dvar, rtol=1e-6, atol=1e-10)
    big = np.concatenate([Xc, p["X"][:30] + 0.01])    # 39 candidates: tile path by size
    np.testing.assert_allclose(model.posterior_variance_gradient(big)[:, :n], dvar, rtol=1e-6, atol=1e-10)
    # every device utility: MC-EI gradient vs the oracle's literal loop
    ref = R.MultiOutputGPRef("matern52", p["variances"], p["lengthscales"], p["noise"])
    ref.updateModel(p["X"], p["Y"])
    mu, sig = ref.posterior_mean(Xc), np.sqrt(ref.posterior_variance(Xc))
    rdm, rdv = ref.posterior_mean_gradient(Xc), ref.posterior_variance_gradient(Xc)
    mu_eval = ref.posterior_mean_at_evaluated_points()
    for util, support, prob, params in (("neg_exp_cos", np.ones((1, 1)), np.ones(1), np.array([1.0, 2.0, 5.0])),
                                        ("linear", np.array([[0.5, -0.2, 0.1]]), np.ones(1), None),
                                        ("neg_sq_dist", np.array([[0.1, 0.2, 0.3], [0.0, -0.3, 0.2]]), np.array([0.5, 0.5]), None)):
        U = B.Utility(parameter_dist=B.ParameterDistribution(support=support, prob_dist=prob), device=util, device_params=params)
        acq = B.uEI_noiseless(model, None, utility=U)
        acq.W_samples = p["W"]
        a, da = acq._compute_acq_withGradients(Xc)
        ra, rda = R.mc_acq_with_gradient(mu, sig, rdm, rdv, mu_eval, p["W"], util, support, prob, util_params=params)
        np.testing.assert_allclose(a, ra, rtol=1e-5, atol=1e-10)
        np.testing.assert_allclose(da, rda, rtol=1e-4, atol=1e-8)


# BASELINE configs[4] shape (m=8 Matern-5/2 ARD, N=8192, d=12, S=4096, uEI utility path) in fp64:
# oracle parity on two of the eight outputs (CPU fits are the slow part) + whole-model properties.
def test_config5_shape_fp64(B):
    N, d, m, C, S = 8192, 12, 8, 2048, 4096
    p = R.synthetic_problem(N, d, m, C, S, 1239, noise=1e-4)
    model = _model(B, "matern52", p["X"], p["Y"], p["variances"], p["lengthscales"], p["noise"])
    assert np.all(model.jitter == 0.0)
    mean, var = model.predict(p["Xc"])
    assert var.min() >= 1e-10 and np.isfinite(mean).all()
    sl = slice(0, 256)
    for j in (0, 7):
        fit = R.GPFit("matern52", p["X"], p["Y"][j], p["variances"][j], p["lengthscales"][j], p["noise"][j])
        rm, rv = fit.predict(p["Xc"][sl])
        np.testing.assert_allclose(mean[j, sl], rm[:, 0], rtol=1e-5, atol=1e-5)
        assert np.abs(var[j, sl] - rv[:, 0]).max() <= 1e-5 * 1.0 + 1e-10
        np.testing.assert_allclose(var[j, sl], rv[:, 0], rtol=1e-4)
        np.testing.assert_allclose(model.log_marginal[j], fit.log_marginal, rtol=1e-8)
    theta = np.array([[1.0]])
    U = B.Utility(parameter_dist=B.ParameterDistribution(support=theta, prob_dist=np.ones(1)), device="rosenbrock")
    acq = B.uEI_noiseless(model, None, utility=U)
    acq.W_samples = p["W"]
    a = acq._compute_acq(p["Xc"])
    assert a.shape == (C, 1) and a.min() >= 0.0 and np.isfinite(a).all()
    top = acq.select_anchors(16)
    np.testing.assert_array_equal(top, np.argsort(-a[:, 0], kind="stable")[:16])
    halves = np.concatenate([acq._compute_acq(p["Xc"][: C // 2]), acq._compute_acq(p["Xc"][C // 2:])])
    np.testing.assert_array_equal(a, halves)


# BASELINE configs[2] at FULL size (m=4 RBF, N=4096, d=8, S=1024, C=65536): oracle parity on a slice,
# plus size-independent properties over the whole batch.
def test_config3_full_size(B):
    N, d, m, C, S = 4096, 8, 4, 65536, 1024
    p = R.synthetic_problem(N, d, m, C, S, 1237)
    model = _model(B, "rbf", p["X"], p["Y"], p["variances"], p["lengthscales"], p["noise"])
    theta = np.array([[0.2 * (j + 1) for j in range(m)]])
    U = B.Utility(parameter_dist=B.ParameterDistribution(support=theta, prob_dist=np.ones(1)), device="neg_sq_dist")
    acq = B.uEI_noiseless(model, None, utility=U)
    acq.W_samples = p["W"]
    a = acq._compute_acq(p["Xc"])
    assert a.shape == (C, 1) and a.min() >= 0.0 and np.isfinite(a).all()
    top = acq.select_anchors(16)
    np.testing.assert_array_equal(top, np.argsort(-a[:, 0], kind="stable")[:16])
    # sharding invariance (what the 8-GPU run relies on): every eighth evaluated alone is bit-identical
    for r in (0, 3, 7):
        lo, hi = r * C // 8, (r + 1) * C // 8
        np.testing.assert_array_equal(acq._compute_acq(p["Xc"][lo:hi]), a[lo:hi])
    # chunked evaluation (4 passes) is bit-identical too
    model.set_option("chunk", 16384)
    np.testing.assert_array_equal(acq._compute_acq(p["Xc"]), a)
    model.set_option("chunk", 65536)
    # oracle parity on the slice that holds the arg-max and on the first 128 candidates
    ref = R.MultiOutputGPRef("rbf", p["variances"], p["lengthscales"], p["noise"])
    ref.updateModel(p["X"], p["Y"])
    idx = np.concatenate([np.arange(128), top])
    r, _, _ = R.batch_uEI(ref, p["Xc"][idx], p["W"], "neg_sq_dist", theta, np.ones(1), "EI")
    # at cond(Ky) ~ 4e9 the posterior mean itself is only defined to ~1e-8 in fp64 (|alpha| ~ 1e6 times 1-ulp
    # kernel values; the reference's own batch and one-at-a-time paths differ by 9e-8 relative already at N=64),
    # so small acquisition values get an absolute floor of 1e-6 x the batch maximum on top of the 1e-5 relative gate
    np.testing.assert_allclose(a[idx], r, rtol=1e-5, atol=1e-6 * r.max())
    assert np.argmax(a[idx]) == np.argmax(r)
    mean, var = model.predict(p["Xc"][idx])
    rm, rv = ref.predict(p["Xc"][idx])
    np.testing.assert_allclose(mean, rm, rtol=1e-5, atol=1e-5)
    rel = np.abs(var - rv) / rv
    print("config3 variance: max rel err %.3e (values %.2e..%.2e)" % (rel.max(), rv.min(), rv.max()))
    assert rel.max() < 1e-4 and np.abs(var - rv).max() <= 1e-5 + 1e-10


# fp32 variance contraction (option predict_f32, the arithmetic BASELINE configs[4] names): K* and the
# inverse factor are rounded to fp32 and contracted with fp32 MFMA; fit and mean stay fp64.
# Documented tolerance: |dvar| <= 2e-5 sigma_f^2 against the fp64 oracle (fp32 cannot hold the
# cancellation sigma_f^2 - ||v||^2 any tighter: eps_f32 x sqrt(N) x ||v||^2), mean bit-identical to fp64.
@pytest.mark.parametrize("N,d,m,kind", [(1000, 6, 2, "rbf"), (2048, 12, 3, "matern52")])
def test_predict_f32(B, N, d, m, kind):
    C = 700
    p = R.synthetic_problem(N, d, m, C, 64, 4000 + N, noise=1e-4)
    model = _model(B, kind, p["X"], p["Y"], p["variances"], p["lengthscales"], p["noise"])
    mean64, var64 = model.predict(p["Xc"])
    model.set_option("predict_f32", 1)
    mean32, var32 = model.predict(p["Xc"])
    np.testing.assert_array_equal(mean32, mean64)
    err = np.abs(var32 - var64).max()
    print("f32 variance contraction: max abs err %.3e (var %.2e..%.2e)" % (err, var64.min(), var64.max()))
    assert err <= 2e-5 and var32.min() >= 1e-10
    # acquisition through the fp32 path stays close where the variance is resolved
    theta = np.array([[0.1 * (j + 1) for j in range(m)]])
    U = B.Utility(parameter_dist=B.ParameterDistribution(support=theta, prob_dist=np.ones(1)), device="neg_sq_dist")
    acq = B.uEI_noiseless(model, None, utility=U)
    acq.W_samples = p["W"]
    a32 = acq._compute_acq(p["Xc"])
    model.set_option("predict_f32", 0)
    a64 = acq._compute_acq(p["Xc"])
    # (|dvar| of 6e-6 on variances of 1e-4 .. 8e-4 is a few per cent of sigma: the acquisition follows it at the per-cent level;
    # which side of 5e-3 of the maximum it lands on depends on the fp32 summation pattern)
    assert np.abs(a32 - a64).max() <= 2e-2 * max(a64.max(), 1e-12) + 1e-9
    # sharding invariance also holds in fp32
    model.set_option("predict_f32", 1)
    np.testing.assert_array_equal(np.concatenate([acq._compute_acq(p["Xc"][:300]), acq._compute_acq(p["Xc"][300:])]), a32)
    # a batch large enough for the 256-row three-buffer fp32 kernel: bit-identical to the 128-row kernel (option swizzle = 0),
    # so a candidate's numbers still do not depend on the size of the batch it travels in
    pb = R.synthetic_problem(N, d, m, 2400, 64, 4000 + N, noise=1e-4)
    model.set_option("swizzle", 0)
    mean_a, var_a = model.predict(pb["Xc"])
    model.set_option("swizzle", -1)
    mean_b, var_b = model.predict(pb["Xc"])
    np.testing.assert_array_equal(var_a, var_b)
    np.testing.assert_array_equal(np.concatenate([model.predict(pb["Xc"][:300])[1], model.predict(pb["Xc"][300:])[1]], axis=1), var_b)
    model.set_option("predict_f32", 0)
    _, var64b = model.predict(pb["Xc"])
    assert np.abs(var_b - var64b).max() <= 2e-5


# randomised shapes: tiny / ragged N, d = 1 ... 12, m = 1 ... 5, every kernel family, against the oracle
@pytest.mark.parametrize("seed", list(range(12)))
def test_random_shapes(B, seed):
    rng = np.random.RandomState(1000 + seed)
    N = int(rng.choice([1, 2, 3, 17, 64, 127, 128, 129, 200, 300]))
    d = int(rng.randint(1, 13))
    m = int(rng.randint(1, 6))
    C = int(rng.choice([1, 5, 16, 17, 100, 257]))
    kind = ["rbf", "se", "matern52", "matern32"][seed % 4]
    iso = bool(rng.randint(0, 2))
    X = rng.uniform(size=(N, d))
    Ys = [rng.normal(size=(N, 1)) for _ in range(m)]
    Xc = rng.uniform(-0.2, 1.2, size=(C, d))
    variances = list(rng.uniform(0.5, 2.0, size=m))
    ls = [np.array([rng.uniform(0.3, 1.5)]) if iso else rng.uniform(0.3, 1.5, size=d) for _ in range(m)]
    noises = list(10.0 ** rng.uniform(-6, -2, size=m))
    model = _model(B, kind, X, Ys, variances, ls, noises)
    ref = R.MultiOutputGPRef(kind, variances, ls, noises)
    ref.updateModel(X, Ys)
    mean, var = model.predict(Xc)
    rm, rv = ref.predict(Xc)
    np.testing.assert_allclose(mean, rm, rtol=1e-6, atol=1e-7)
    assert np.abs(var - rv).max() <= 1e-8 * max(variances)
    np.testing.assert_allclose(model.posterior_variance_noiseless(Xc), ref.posterior_variance_noiseless(Xc), rtol=1e-5, atol=1e-8)
    np.testing.assert_allclose(model.log_marginal, [o.log_marginal for o in ref.output], rtol=1e-9, atol=1e-9)
    np.testing.assert_allclose(model.posterior_mean_at_evaluated_points(), ref.posterior_mean_at_evaluated_points(), rtol=1e-6, atol=1e-7)
    dm, dv = model.posterior_mean_gradient(Xc), model.posterior_variance_gradient(Xc)
    np.testing.assert_allclose(dm, ref.posterior_mean_gradient(Xc), rtol=1e-5, atol=1e-6)
    np.testing.assert_allclose(dv, ref.posterior_variance_gradient(Xc), rtol=1e-4, atol=1e-7)
    W = rng.normal(size=(9, m))
    support, prob = rng.normal(size=(2, m)), np.array([0.3, 0.7])
    U = B.Utility(parameter_dist=B.ParameterDistribution(support=support, prob_dist=prob), device="neg_sq_dist")
    acq = B.uEI_noiseless(model, None, utility=U)
    acq.W_samples = W
    a = acq._compute_acq(Xc)
    r, _ = R.mc_acq(ref.posterior_mean(Xc), np.sqrt(ref.posterior_variance(Xc)), ref.posterior_mean_at_evaluated_points(), W,
                    "neg_sq_dist", support, prob, "EI")
    np.testing.assert_allclose(a, r, rtol=1e-5, atol=1e-9)
    k = min(16, C)
    np.testing.assert_array_equal(acq.select_anchors(k), np.argsort(-a[:, 0], kind="stable")[:k])


# log-marginal hyper-gradients (numerical core) vs the reference's numbers (golden)
@pytest.mark.parametrize("tag,kind", [("se_ard", "se"), ("se_iso", "se"), ("rbf_ard", "rbf"), ("rbf_iso", "rbf"), ("m52_ard", "matern52"),
                                      ("m32_iso", "matern32")])
def test_hyper_gradients_golden(B, golden, tag, kind):
    g = golden("hypergrads")
    X, Y, ls, var, noise = g[tag + "_X"], g[tag + "_Y"], g[tag + "_ls"], float(g[tag + "_var"]), float(g[tag + "_noise"])
    model = _model(B, kind, X, [Y, 2.0 * Y + 1.0], [var, var], [ls, ls], [noise, noise])
    np.testing.assert_allclose(model.log_likelihood()[0], g[tag + "_lml"], rtol=1e-9)
    dv, dl, dn = model.log_likelihood_gradients()
    assert dv.shape == (2,) and dl.shape == (2, X.shape[1]) and dn.shape == (2,)
    np.testing.assert_allclose(dv[0], g[tag + "_dvar"], rtol=1e-6)
    np.testing.assert_allclose(dn[0], g[tag + "_dnoise"], rtol=1e-6)
    want = g[tag + "_dls"]
    got = dl[0] if want.size > 1 else np.atleast_1d(dl[0].sum())     # isotropic: one lengthscale = sum over d
    np.testing.assert_allclose(got, want, rtol=1e-6, atol=1e-8)
    # second output (scaled targets) against the oracle
    fit = R.GPFit(kind, X, 2.0 * Y + 1.0, var, ls, noise)
    rv, rl, rn = fit.lml_gradients()
    np.testing.assert_allclose(dv[1], rv, rtol=1e-6)
    np.testing.assert_allclose(dn[1], rn, rtol=1e-6)
    np.testing.assert_allclose(dl[1] if rl.size > 1 else dl[1].sum(), rl if rl.size > 1 else rl[0], rtol=1e-6, atol=1e-8)


def test_hyper_gradients_multi_tile(B):
    N, d, m = 700, 5, 2
    p = R.synthetic_problem(N, d, m, 8, 4, 606, noise=1e-3)
    model = _model(B, "rbf", p["X"], p["Y"], p["variances"], p["lengthscales"], p["noise"])
    dv, dl, dn = model.log_likelihood_gradients()
    for j in range(m):
        rv, rl, rn = R.GPFit("rbf", p["X"], p["Y"][j], p["variances"][j], p["lengthscales"][j], p["noise"][j]).lml_gradients()
        np.testing.assert_allclose(dv[j], rv, rtol=1e-6)
        np.testing.assert_allclose(dl[j], rl, rtol=1e-6, atol=1e-7)
        np.testing.assert_allclose(dn[j], rn, rtol=1e-6)


# incremental updateModel: targets-only refresh and rank-1 append equal a from-scratch fit (N = 120 .. 135, one padding
# boundary).  The other tile / grid boundaries, schedules, reused buffers, derived copies of R, long chains and the refusals:
# tests/test_gpu_incremental.py
def test_incremental_update(B):
    d, m, C = 4, 3, 200
    p = R.synthetic_problem(140, d, m, C, 8, 909, noise=1e-4)
    X, Ys = p["X"], p["Y"]
    model = B.multi_outputGP(m, kernel=[_kern(B, "matern52", d, p["variances"][j], p["lengthscales"][j]) for j in range(m)],
                             noise_var=list(p["noise"]), fixed_hyps=True)
    n0 = 120
    model.updateModel(X[:n0], [y[:n0] for y in Ys])
    calls = {"fit": 0}
    orig_fit = model._fit

    def counting_fit():
        calls["fit"] += 1
        orig_fit()
    model._fit = counting_fit

    def check(n, Yl):
        ref = R.MultiOutputGPRef("matern52", p["variances"], p["lengthscales"], p["noise"])
        ref.updateModel(X[:n], Yl)
        mean, var = model.predict(p["Xc"])
        rm, rv = ref.predict(p["Xc"])
        np.testing.assert_allclose(mean, rm, rtol=1e-6, atol=1e-7)
        assert np.abs(var - rv).max() <= 1e-9
        np.testing.assert_allclose(model.log_marginal, [o.log_marginal for o in ref.output], rtol=1e-9)
        np.testing.assert_allclose(model.posterior_mean_at_evaluated_points(), ref.posterior_mean_at_evaluated_points(), rtol=1e-6, atol=1e-7)
        L, alpha = model.get_factor(m - 1)
        np.testing.assert_allclose(L, ref.output[m - 1].L, rtol=1e-6, atol=1e-9)
        dm, dv = model.posterior_mean_gradient(p["Xc"][:5]), model.posterior_variance_gradient(p["Xc"][:5])
        np.testing.assert_allclose(dm, ref.posterior_mean_gradient(p["Xc"][:5]), rtol=1e-5, atol=1e-6)
        np.testing.assert_allclose(dv, ref.posterior_variance_gradient(p["Xc"][:5]), rtol=1e-4, atol=1e-8)
        dvh, dlh, dnh = model.log_likelihood_gradients()
        rvh, rlh, rnh = ref.output[0].lml_gradients()
        np.testing.assert_allclose([dvh[0], dnh[0]], [rvh, rnh], rtol=1e-6)
        np.testing.assert_allclose(dlh[0], rlh, rtol=1e-6, atol=1e-8)

    # same inputs, new targets -> no refit
    Y2 = [y[:n0] * 1.5 - 0.3 for y in Ys]
    model.updateModel(X[:n0], Y2)
    assert calls["fit"] == 0
    check(n0, Y2)
    # one observation at a time, through the 128-row padding boundary (a refit happens exactly there)
    for n in range(n0 + 1, 136):
        model.updateModel(X[:n], [y[:n] for y in Ys])
        if n in (121, 127, 128, 129, 135):
            check(n, [y[:n] for y in Ys])
    assert calls["fit"] == 1
    # changed hyper-parameters or changed history -> refit
    Xmod = X[:135].copy()
    Xmod[3, 0] += 0.01
    model.updateModel(np.vstack([Xmod, X[135:136]]), [y[:136] for y in Ys])
    assert calls["fit"] == 2
    model.incremental = False
    model.updateModel(X[:137], [y[:137] for y in Ys])
    assert calls["fit"] == 3



# the <= 16-candidate device path is batch-invariant: a row's value and gradient do not depend on which other
# rows share the call (so refining anchors one at a time or together gives the same iterates)
def test_small_batch_invariance(B):
    N, d, m = 200, 3, 2
    p = R.synthetic_problem(N, d, m, 2000, 32, 515, noise=1e-4)
    model = _model(B, "rbf", p["X"], p["Y"], p["variances"], p["lengthscales"], p["noise"])
    theta = np.array([[0.2, -0.1]])
    U = B.Utility(parameter_dist=B.ParameterDistribution(support=theta, prob_dist=np.ones(1)), device="neg_sq_dist")
    acq = B.uEI_noiseless(model, None, utility=U)
    acq.W_samples = p["W"]
    acq.acquisition_function(p["Xc"])
    anchors = p["Xc"][acq.select_anchors(16)]
    fa, ga = acq.acquisition_function_withGradients(anchors)
    for rows in ([0], [7], [15], [2, 9, 11], list(range(8))):
        f1, g1 = acq.acquisition_function_withGradients(anchors[rows])
        np.testing.assert_array_equal(f1, fa[rows])
        np.testing.assert_array_equal(g1, ga[rows])


# BASELINE configs[1] at full size against the reference's own acquisition values and top-16 selection
def test_config2_golden_selection(B, golden):
    g = golden("e2e")
    N, d, m, C, S = 1024, 6, 4, 8192, 256
    p = R.synthetic_problem(N, d, m, C, S, int(g["cfg2_seed"]))
    model = _model(B, "rbf", p["X"], p["Y"], p["variances"], p["lengthscales"], p["noise"])
    np.testing.assert_allclose(model.log_marginal, g["cfg2_lml"], rtol=1e-8)
    U = B.Utility(parameter_dist=B.ParameterDistribution(support=g["cfg2_theta"], prob_dist=np.ones(1)), device="neg_sq_dist")
    acq = B.uEI_noiseless(model, None, utility=U)
    acq.W_samples = p["W"]
    a = acq._compute_acq(p["Xc"])
    np.testing.assert_allclose(a, g["cfg2_uEI"], rtol=1e-5, atol=1e-7 * g["cfg2_uEI"].max())
    _check_selection_vs_reference(acq.select_anchors(16), g["cfg2_uEI"][:, 0], g["cfg2_sel_uEI"])
    lin = B.Utility(parameter_dist=B.ParameterDistribution(support=np.full((1, m), 1.0 / m), prob_dist=np.ones(1)), linear=True)
    mae = B.maEI(model, None, utility=lin)
    a = mae._compute_acq(p["Xc"])
    np.testing.assert_allclose(a, g["cfg2_maEI"], rtol=1e-5, atol=1e-7 * g["cfg2_maEI"].max())
    _check_selection_vs_reference(mae.select_anchors(16), g["cfg2_maEI"][:, 0], g["cfg2_sel_maEI"])


def _check_selection_vs_reference(sel, ref_acq, ref_sel):
    """Our top-k against the reference's np.argsort(-acq)[:k]: identical index wherever the reference value is
    untied (exact ties -- typically acq == 0 for most of a Monte-Carlo EI batch -- are ordered arbitrarily by the
    reference's quicksort and by lowest index here, so only the values must agree there)."""
    assert sel[0] == ref_sel[0]
    np.testing.assert_allclose(ref_acq[sel], ref_acq[ref_sel], rtol=1e-5, atol=0)
    for i, j in zip(sel, ref_sel):
        if np.sum(ref_acq == ref_acq[j]) == 1:
            assert i == j


# every reduction on the path has a fixed order: two contexts fed the same inputs return bit-identical
# numbers (what "argmax index bit-exact" across ranks and runs rests on)
def test_run_to_run_determinism(B):
    N, d, m, C, S = 700, 5, 3, 3000, 64
    p = R.synthetic_problem(N, d, m, C, S, 2468, noise=1e-5)
    outs = []
    for _ in range(2):
        model = _model(B, "matern52", p["X"], p["Y"], p["variances"], p["lengthscales"], p["noise"])
        U = B.Utility(parameter_dist=B.ParameterDistribution(support=np.array([[0.1, 0.2, 0.3]]), prob_dist=np.ones(1)), device="neg_sq_dist")
        acq = B.uEI_noiseless(model, None, utility=U)
        acq.W_samples = p["W"]
        a = acq._compute_acq(p["Xc"])
        top = acq.select_anchors(16)          # selection refers to the last acquisition batch
        mean, var = model.predict(p["Xc"])
        with pytest.raises(B._ffi.BocfHipError):
            acq.select_anchors(16)            # ... and is refused once the resident batch has been replaced
        L, alpha = model.get_factor(0)
        dm, dv = model.posterior_mean_gradient(p["Xc"][:40]), model.posterior_variance_gradient(p["Xc"][:40])
        outs.append((a, mean, var, L, alpha, dm, dv, model.log_marginal.copy(), top))
    for x, y in zip(*outs):
        np.testing.assert_array_equal(x, y)


# the whole acquisition-optimisation step on the device (score n_starting random starts, top-16
# on the device, all anchors refined together with batched f_df passes) against the reference's flow
# (acquisition_optimizer.py:95-154: np.argsort anchors, one scipy L-BFGS-B per anchor, f at every optimum) on the oracle.
@pytest.mark.parametrize("which", ["maEI", "uEI"])
def test_acquisition_optimizer_vs_reference_flow(B, which):
    import scipy.optimize
    from bocf_amd import acquisition_optimizer as AO
    N, d, m, S = 40, 3, 3, 128
    p = R.synthetic_problem(N, d, m, 8, S, 4242)
    model = _model(B, "rbf", p["X"], p["Y"], p["variances"], p["lengthscales"], p["noise"])
    ref = R.MultiOutputGPRef("rbf", p["variances"], p["lengthscales"], p["noise"])
    ref.updateModel(p["X"], p["Y"])
    mu_eval = ref.posterior_mean_at_evaluated_points()
    bounds = [(0.0, 1.0)] * d
    space = AO.Design_space(bounds=bounds)
    if which == "maEI":
        theta, prob = np.full((1, m), 1.0 / m), np.ones(1)
        U = B.Utility(parameter_dist=B.ParameterDistribution(support=theta, prob_dist=prob), linear=True)
        acq = B.maEI(model, space, optimizer=AO.AcquisitionOptimizer(space, n_starting=400, n_anchor=16), utility=U)

        def ref_f_df(Z):
            Z = np.atleast_2d(Z)
            mean, var = ref.predict(Z)
            a, g = R.ma_acq_with_gradient(mean, var, ref.posterior_mean_gradient(Z), ref.posterior_variance_gradient(Z), mu_eval, theta, prob, "EI")
            return -np.reshape(a, (-1, 1)), -np.reshape(g, Z.shape)
    else:
        theta, prob = np.array([[1.2, -1.0, 1.1]]), np.ones(1)
        U = B.Utility(parameter_dist=B.ParameterDistribution(support=theta, prob_dist=prob), device="neg_sq_dist")
        acq = B.uEI_noiseless(model, space, optimizer=AO.AcquisitionOptimizer(space, n_starting=400, n_anchor=16), utility=U)
        acq.W_samples = p["W"]

        def ref_f_df(Z):
            Z = np.atleast_2d(Z)
            mu, sig = ref.posterior_mean(Z), np.sqrt(ref.posterior_variance(Z))
            a, g = R.mc_acq_with_gradient(mu, sig, ref.posterior_mean_gradient(Z), ref.posterior_variance_gradient(Z), mu_eval, p["W"],
                                          "neg_sq_dist", theta, prob)
            return -np.reshape(a, (-1, 1)), -np.reshape(g, Z.shape)
    # reference flow on the oracle
    np.random.seed(11)
    X0 = AO.samples_multidimensional_uniform(bounds, 400)
    scores = ref_f_df(X0)[0].flatten()
    anchors = X0[np.argsort(scores)[:16]]
    outs = []
    for a in anchors:
        res = scipy.optimize.fmin_l_bfgs_b(lambda x: (float(ref_f_df(x)[0][0, 0]), ref_f_df(x)[1][0]), x0=a, bounds=bounds, maxiter=500, factr=1e6)
        outs.append((np.atleast_2d(res[0]), ref_f_df(res[0])[0][0, 0]))
    x_ref, fx_ref = min(outs, key=lambda t: t[1])
    # device flow through the plug-in surface: acquisition.optimize() (base.py:58-66)
    np.random.seed(11)
    x_min, fx_min = acq.optimize()
    info = acq.optimizer.last_info
    assert x_min.shape == (1, d) and np.shape(fx_min) == (1, 1)
    ref_anchor_scores = np.sort(scores)[:16]
    np.testing.assert_allclose(info["anchor_points_values"], ref_anchor_scores, rtol=1e-5, atol=1e-9 * abs(fx_ref))
    untied = np.array([np.sum(np.isclose(scores, v, rtol=1e-4, atol=0)) == 1 for v in ref_anchor_scores])
    assert untied.sum() >= 8
    np.testing.assert_array_equal(info["anchor_points"][untied], anchors[untied])
    assert fx_min[0, 0] <= fx_ref + 1e-5 * abs(fx_ref)
    if abs(fx_min[0, 0] - fx_ref) <= 1e-5 * abs(fx_ref):
        np.testing.assert_allclose(x_min, x_ref, atol=5e-3)
    # the value reported is the acquisition at the point reported (optimizer.py:464), per the oracle too
    np.testing.assert_allclose(fx_min[0, 0], ref_f_df(x_min)[0][0, 0], rtol=1e-5)
    assert info["f_df_calls"] < 120                     # batched passes, vs several hundred single-point calls


# ---------------------------------------------------------------------------------------------
# hyper-parameter learning (GPModel.updateModel, gpmodel.py:102-128) with device inferences
def _learning_problem(seed=0, N=40, d=2):
    rng = np.random.RandomState(seed)
    X = rng.uniform(size=(N, d))
    Ys = [np.sin(3 * X.sum(1))[:, None], (np.cos(4 * X[:, 0]) + X[:, 1])[:, None] + 0.05 * rng.normal(size=(N, 1)),
          (X[:, 0] * X[:, 1])[:, None]]
    return X, Ys


def _learning_model(B, X, Ys, **kw):
    # output 0: exact_feval (noise fixed at 1e-6); output 1: free noise from 0.01 Var(Y); output 2: given noise (fixed)
    model = B.multi_outputGP(3, exact_feval=[True, False, False], noise_var=[None, None, 1e-3], ARD=[True, False, True],
                             n_samples=kw.pop("n_samples", 3), fixed_hyps=False)
    for k, v in kw.items():
        setattr(model, k, v)
    return model


def test_hyper_inference_matches_oracle(B):
    from bocf_amd import hyper as H
    X, Ys = _learning_problem()
    model = _learning_model(B, X, Ys)
    model._X, model._Y = X, Ys
    model._create_sampler_state()
    outs = model._sampler_outputs
    assert [o.param_array.size for o in outs] == [4, 3, 4] and [bool(o.fixed[-1]) for o in outs] == [True, False, True]
    np.testing.assert_allclose(outs[1].param_array[-1], 0.01 * np.var(Ys[1]))           # gpmodel.py:64
    sampler = H.LockstepSampler(outs, model._infer, X.shape[1])
    for trial in range(2):
        obj, tg = sampler.evaluate()
        for j, o in enumerate(outs):
            p = o.param_array
            ref = R.GPHyperRef("se", X, Ys[j], p[0], p[1:-1], p[-1], bool(o.fixed[-1]))
            np.testing.assert_allclose(obj[j], ref.objective_function(), rtol=1e-8)
            g = ref._transform_gradients(ref.objective_function_gradients())
            np.testing.assert_allclose(tg[j], g, rtol=1e-5, atol=1e-6 * np.abs(g).max())
        for o in outs:                                                                   # second trial: other parameters
            o.optimizer_array = o.optimizer_array + 0.3
    assert sampler.n_inferences == 2


@pytest.mark.parametrize("path", ["lockstep", "resident"])
@pytest.mark.parametrize("tag,kind", [("se_ard_fixed", "se"), ("rbf_iso_free", "rbf"), ("m52_ard_free", "matern52")])
def test_device_hmc_chain_golden(B, golden, tag, kind, path):
    """HMC with device inferences against the chain the reference's own hmc.py produced (golden): the lockstep host loop (one batched
    device inference per leapfrog step) and the device-RESIDENT chain (bocf_hmc: the whole chain in one launch)."""
    from bocf_amd import hyper as H
    g = golden("hyper")
    X, Y, th, fixed = g[tag + "_X"], g[tag + "_Y"], g[tag + "_theta0"], g[tag + "_fixed"]
    d = X.shape[1]
    cls = {"se": B.kern.SE, "rbf": B.kern.RBF, "matern52": B.kern.Matern52}[kind]
    ard = th.size - 2 == d and d > 1
    model = B.multi_outputGP(1, kernel=[cls(d, variance=th[0], lengthscale=th[1:-1], ARD=ard)], fixed_hyps=False, n_samples=2,
                             exact_feval=[bool(fixed[-1]) and th[-1] == 1e-6], noise_var=[None if th[-1] == 1e-6 else th[-1]])
    model._X, model._Y = X, [Y]
    model._create_sampler_state()
    out = model._sampler_outputs[0]
    out.fixed[-1] = bool(fixed[-1])                          # the golden "free" cases start from a given noise value
    np.testing.assert_allclose(out.param_array, th, rtol=1e-15)
    ns, iters, step = int(g[tag + "_num_samples"]), int(g[tag + "_hmc_iters"]), float(g[tag + "_stepsize"])
    np.random.seed(int(g[tag + "_seed"]))
    P = int(np.sum(~out.fixed))
    mom, u = np.empty((ns, P)), np.empty(ns)
    for i in range(ns):                                      # hmc.py:43,55
        mom[i] = np.random.multivariate_normal(np.zeros(P), np.eye(P))
        u[i] = np.random.rand()
    sampler = H.LockstepSampler([out], model._infer, d, device_hmc=model._device_hmc if path == "resident" else None)
    chain = sampler.hmc([mom], [u], hmc_iters=iters, stepsize=step)[0]
    np.testing.assert_allclose(chain, g[tag + "_chain"], rtol=1e-5, atol=1e-8)
    np.testing.assert_allclose(out.param_array, g[tag + "_theta_end"], rtol=1e-5, atol=1e-8)
    assert sampler.n_inferences <= 1 + ns * iters


def test_update_model_learning_vs_oracle_flow(B):
    """multi_outputGP(fixed_hyps=False).updateModel == gpmodel.py:102-128 per output, in the reference's RNG order."""
    X, Ys = _learning_problem(1)
    cfg = dict(n_burnin=4, subsample_interval=2, leapfrog_steps=3, step_size=0.02, max_iters=0)
    model = _learning_model(B, X, Ys, n_samples=3, **cfg)
    np.random.seed(21)
    model.updateModel(X, Ys)
    after = np.random.rand()
    info = model.last_update_info
    assert info["num_samples"] == 10 and info["hmc_inferences"] <= 10 * 3 + 1
    # the same flow on the oracle, output after output (max_iters=0: no optimiser step, so both start HMC from the same point)
    np.random.seed(21)
    specs = [(1.0, [1.0, 1.0], 1e-6, True), (1.0, [1.0], 0.01 * np.var(Ys[1]), False), (1.0, [1.0, 1.0], 1e-3, True)]
    ref_samples = []
    for j, sp in enumerate(specs):
        ref = R.GPHyperRef("se", X, Ys[j], *sp)
        ref.param_array[:] = ref.param_array * (1. + np.random.randn(ref.param_array.size) * 0.01)
        ss = R.hmc_sample(ref, 10, 3, 0.02)
        ref_samples.append(ss[4::2])
    assert after == np.random.rand()
    for j in range(3):
        np.testing.assert_allclose(model.hmc_samples[j], ref_samples[j], rtol=1e-5, atol=1e-9)
    assert model.number_of_hyps_samples() == 3
    # every hyper-sample is a full model on the device: predictions per set_hyperparameters(h) vs the oracle
    Xc = np.random.RandomState(5).uniform(size=(37, 2))
    refs = []
    for h in range(3):
        inst = model._instances[h]
        ref = R.MultiOutputGPRef("se", [i[0] for i in inst], [i[1] for i in inst], [i[2] for i in inst])
        ref.updateModel(X, Ys)
        refs.append(ref)
        assert inst[0][2] == 1e-6 and inst[2][2] == 1e-3                # fixed noises keep their constrained value
        np.testing.assert_allclose(inst[1][1], np.full(2, model.hmc_samples[1][h][1]))   # isotropic lengthscale repeated
        model.set_hyperparameters(h)
        mean, var = model.predict(Xc)
        rm, rv = ref.predict(Xc)
        np.testing.assert_allclose(mean, rm, rtol=1e-5, atol=1e-6)
        np.testing.assert_allclose(var, rv, rtol=1e-4, atol=1e-8)
        np.testing.assert_allclose(model.posterior_mean_at_evaluated_points(), ref.posterior_mean_at_evaluated_points(), rtol=1e-5, atol=1e-6)
        np.testing.assert_allclose(model.posterior_mean_gradient(Xc[:5]), ref.posterior_mean_gradient(Xc[:5]), rtol=1e-4, atol=1e-6)
        np.testing.assert_allclose(model.log_likelihood(), [o.log_marginal for o in ref.output], rtol=1e-7)
        pars = model.get_model_parameters()
        assert pars[1].shape == (1, 4) and pars[1][0, 0] == inst[1][0]
    with pytest.raises(IndexError):
        model.set_hyperparameters(3)
    # ---- acquisitions average over the hyper-samples on the device
    means = [r.predict(Xc)[0] for r in refs]
    vars_ = [r.predict(Xc)[1] for r in refs]
    mu_evals = [r.posterior_mean_at_evaluated_points() for r in refs]
    theta, prob = np.array([[0.5, 0.2, 0.3], [0.1, 0.6, 0.3]]), np.array([0.4, 0.6])
    U = B.Utility(parameter_dist=B.ParameterDistribution(support=theta, prob_dist=prob), linear=True)
    for cls, kind in ((B.maEI, "EI"), (B.maPI, "PI")):
        acq = cls(model, None, utility=U)
        assert acq.n_hyps_samples == 3
        a = acq._compute_acq(Xc)[:, 0]
        np.testing.assert_allclose(a, R.ma_acq_hyper(means, vars_, mu_evals, theta, prob, kind), rtol=1e-5, atol=1e-9)
        assert model._current_h == 2                                   # the h-loop leaves the last hyper-sample selected
    # maEI value + gradient: the gradient of the h-averaged acquisition (finite differences through the device path)
    acq = B.maEI(model, None, utility=U)
    a, da = acq._compute_acq_withGradients(Xc[:6])
    np.testing.assert_allclose(a[:, 0], R.ma_acq_hyper([mm[:, :6] for mm in means], [vv[:, :6] for vv in vars_], mu_evals, theta, prob, "EI"),
                               rtol=1e-5, atol=1e-9)
    hstep = 1e-6
    for q in range(2):
        Xp, Xm = Xc[:6].copy(), Xc[:6].copy()
        Xp[:, q] += hstep
        Xm[:, q] -= hstep
        fd = (acq._compute_acq(Xp) - acq._compute_acq(Xm))[:, 0] / (2 * hstep)
        np.testing.assert_allclose(da[:, q], fd, rtol=2e-4, atol=1e-6 * np.abs(da).max())
    # uEI: best-so-far from the hyper-sample current on entry (uEI_noiseless.py:66), here h = 1, then h = 2 (left by the loop)
    Um = B.Utility(parameter_dist=B.ParameterDistribution(support=np.array([[0.9, 1.1, 0.4]]), prob_dist=np.ones(1)), device="neg_sq_dist")
    uacq = B.uEI_noiseless(model, None, utility=Um)
    W = np.random.RandomState(9).normal(size=(64, 3))
    uacq.W_samples = W
    mus = [r.posterior_mean(Xc) for r in refs]
    sigs = [np.sqrt(r.posterior_variance(Xc)) for r in refs]
    for entry_h in (1, 2):
        model.set_hyperparameters(entry_h)
        a = uacq._compute_acq(Xc)[:, 0]
        ra = R.mc_acq_hyper(mus, sigs, mu_evals[entry_h], W, "neg_sq_dist", np.array([[0.9, 1.1, 0.4]]), np.ones(1), "EI")
        np.testing.assert_allclose(a, ra, rtol=1e-5, atol=1e-9 * max(ra.max(), 1e-30))
        assert model._current_h == 2
    assert a.max() > 0
    model.set_hyperparameters(0)
    a0, da0 = uacq._compute_acq_withGradients(Xc[:6])
    ra0 = R.mc_acq_hyper([mm[:, :6] for mm in mus], [ss[:, :6] for ss in sigs], mu_evals[0], W, "neg_sq_dist", np.array([[0.9, 1.1, 0.4]]),
                         np.ones(1), "EI")
    np.testing.assert_allclose(a0[:, 0], ra0, rtol=1e-5, atol=1e-12)
    # EI (single-output specialisation) averages over n_hyps_samples = 1 hyper-sample only (EI.py:35)
    m1 = B.multi_outputGP(1, exact_feval=[True], fixed_hyps=False, n_samples=2)
    for k, v in cfg.items():
        setattr(m1, k, v)
    np.random.seed(3)
    m1.updateModel(X, [Ys[0]])
    e = B.EI(m1, None, utility=B.Utility(parameter_dist=B.ParameterDistribution(support=np.ones((1, 1)), prob_dist=np.ones(1)), linear=True))
    inst = m1._instances[0]
    r0 = R.MultiOutputGPRef("se", [inst[0][0]], [inst[0][1]], [inst[0][2]])
    r0.updateModel(X, [Ys[0]])
    mean0, var0 = r0.predict(Xc)
    want = R.ma_acq(mean0, var0, r0.posterior_mean_at_evaluated_points(), np.ones((1, 1)), np.ones(1), "EI")[0][:, 0]
    np.testing.assert_allclose(e._compute_acq(Xc)[:, 0], want, rtol=1e-5, atol=1e-10)


def test_update_model_learning_full_flow_properties(B):
    """Optimiser + HMC with the reference's flow at reduced lengths: the optimiser lowers every output's objective, HMC
    accepts, a second updateModel continues from the sampler state, same seed => same samples."""
    from bocf_amd import hyper as H
    X, Ys = _learning_problem(2, N=60, d=3)
    cfg = dict(n_burnin=6, subsample_interval=2, leapfrog_steps=5, step_size=0.02, max_iters=200)
    runs = []
    for rep in range(2):
        model = _learning_model(B, X, Ys, n_samples=4, **cfg)
        np.random.seed(8)
        model.updateModel(X, Ys)
        runs.append([s.copy() for s in model.hmc_samples])
    for a, b in zip(*runs):
        np.testing.assert_array_equal(a, b)
    info = model.last_update_info
    assert info["optimizer_inferences"] <= 3 * 200 and np.all(info["accepted"] > 0)
    # objective at the optimiser's result (re-run it alone) is below the starting objective for every output
    m2 = _learning_model(B, X, Ys, n_samples=4, **cfg)
    m2._X, m2._Y = X, Ys
    m2._create_sampler_state()
    s2 = H.LockstepSampler(m2._sampler_outputs, m2._infer, 3)
    f0 = s2.evaluate()[0].copy()
    s2.optimize(200)
    f1 = s2.evaluate()[0]
    assert np.all(f1 < f0 - 1.0)
    for j, sp in enumerate([(1.0, [1.0] * 3, 1e-6, True), (1.0, [1.0], 0.01 * np.var(Ys[1]), False), (1.0, [1.0] * 3, 1e-3, True)]):
        ref = R.GPHyperRef("se", X, Ys[j], *sp)
        R.optimize_hyper(ref, 200)
        fr = ref.objective_function()
        assert f1[j] <= fr + 1e-3 * max(1.0, abs(fr)), (j, f1[j], fr)
    # one more observation: the sampler continues from where it stood (gpmodel.py:109-112), all hyper-samples refitted
    Xn = np.vstack([X, [[0.3, 0.6, 0.9]]])
    Yn = [np.vstack([y, [[0.1 * (j + 1)]]]) for j, y in enumerate(Ys)]
    before = [o.param_array.copy() for o in model._sampler_outputs]
    model.updateModel(Xn, Yn)
    assert model.posterior_mean_at_evaluated_points().shape == (3, 61)
    assert any(not np.array_equal(b, o.param_array) for b, o in zip(before, model._sampler_outputs))
    mean, var = model.predict(Xn[-3:])
    assert mean.shape == (3, 3) and np.all(var > 0)
    np.testing.assert_allclose(mean[0, -1], 0.1, atol=5e-2)          # exact_feval output interpolates its new observation


def test_bo_loop_example_composes(B):
    """examples/bo_loop.py: learning model + uEI over the hyper-samples + device acquisition optimiser, three iterations."""
    import importlib.util
    import os
    spec = importlib.util.spec_from_file_location("bo_loop", os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "examples", "bo_loop.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    X, Y, hist = mod.run(iterations=3, n_starting=512, quick=True, seed=4, verbose=False)
    assert X.shape == (9, 2) and all(y.shape == (9, 1) for y in Y)
    assert np.all(X >= 0) and np.all(X <= 1)
    assert hist == sorted(hist)                                     # best-so-far utility never decreases
    X2, _, hist2 = mod.run(iterations=3, n_starting=512, quick=True, seed=4, verbose=False)
    np.testing.assert_array_equal(X, X2)                            # same seed, same trajectory (host RNG only)


def test_learning_mode_more_cases(B):
    """Learning mode beyond the main flow test: Matern-5/2 user kernels, 12 hyper-samples (acquisitions use the first
    min(10, H), maEI.py:35), uPI / maPI (+gradient) over hyper-samples, d = 1 / m = 1, pickling."""
    import pickle
    rng = np.random.RandomState(12)
    N, d, m = 30, 2, 2
    X = rng.uniform(size=(N, d))
    Ys = [np.sin(4 * X[:, :1]) + X[:, 1:], np.cos(3 * X[:, 1:]) * X[:, :1]]
    kern = [B.kern.Matern52(d, variance=1.2, lengthscale=[0.6, 0.8], ARD=True), B.kern.Matern52(d, variance=0.8, lengthscale=0.7)]
    model = B.multi_outputGP(m, kernel=kern, noise_var=[1e-4, None], n_samples=12, fixed_hyps=False)
    model.n_burnin, model.subsample_interval, model.leapfrog_steps, model.step_size, model.max_iters = 3, 1, 3, 0.02, 5
    np.random.seed(2)
    model.updateModel(X, Ys)
    assert len(model._instances) == 12 and model.hmc_samples[0].shape == (12, 3) and model.hmc_samples[1].shape == (12, 3)
    refs = []
    for h in range(12):
        inst = model._instances[h]
        r = R.MultiOutputGPRef("matern52", [i[0] for i in inst], [i[1] for i in inst], [i[2] for i in inst])
        r.updateModel(X, Ys)
        refs.append(r)
    Xc = rng.uniform(size=(21, d))
    model.set_hyperparameters(11)
    mean, var = model.predict(Xc)
    rm, rv = refs[11].predict(Xc)
    np.testing.assert_allclose(mean, rm, rtol=1e-5, atol=1e-6)
    np.testing.assert_allclose(var, rv, rtol=1e-4, atol=1e-9)
    np.testing.assert_allclose(model.posterior_variance_gradient(Xc[:4]), refs[11].posterior_variance_gradient(Xc[:4]), rtol=1e-4, atol=1e-7)
    theta, prob = np.array([[0.7, 0.3]]), np.ones(1)
    U = B.Utility(parameter_dist=B.ParameterDistribution(support=theta, prob_dist=prob), linear=True)
    means = [r.predict(Xc)[0] for r in refs[:10]]
    vars_ = [r.predict(Xc)[1] for r in refs[:10]]
    mu_evals = [r.posterior_mean_at_evaluated_points() for r in refs[:10]]
    pi = B.maPI(model, None, utility=U)
    assert pi.n_hyps_samples == 10
    a = pi._compute_acq(Xc)[:, 0]
    np.testing.assert_allclose(a, R.ma_acq_hyper(means, vars_, mu_evals, theta, prob, "PI"), rtol=1e-5, atol=1e-12)
    assert model._current_h == 9
    a2, da = pi._compute_acq_withGradients(Xc[:5])
    np.testing.assert_allclose(a2[:, 0], a[:5], rtol=1e-9, atol=1e-14)
    hstep = 1e-6
    for q in range(d):
        Xp, Xm = Xc[:5].copy(), Xc[:5].copy()
        Xp[:, q] += hstep
        Xm[:, q] -= hstep
        fd = (pi._compute_acq(Xp) - pi._compute_acq(Xm))[:, 0] / (2 * hstep)
        np.testing.assert_allclose(da[:, q], fd, rtol=5e-4, atol=1e-6 * max(np.abs(da).max(), 1e-30))
    Um = B.Utility(parameter_dist=B.ParameterDistribution(support=np.array([[1.0, 0.2]]), prob_dist=np.ones(1)), device="neg_sq_dist")
    upi = B.uPI(model, None, utility=Um)
    W = rng.normal(size=(200, m))
    upi.W_samples = W
    model.set_hyperparameters(3)
    a = upi._compute_acq(Xc)[:, 0]
    mus = [r.posterior_mean(Xc) for r in refs[:10]]
    sigs = [np.sqrt(r.posterior_variance(Xc)) for r in refs[:10]]
    ra = R.mc_acq_hyper(mus, sigs, refs[3].posterior_mean_at_evaluated_points(), W, "neg_sq_dist", np.array([[1.0, 0.2]]), np.ones(1), "PI")
    np.testing.assert_allclose(a, ra, rtol=0, atol=1.0 / (10 * 200) + 1e-12)       # indicator counts: at most one borderline sample
    # pickling drops the device handle; the copy refits its hyper-samples lazily and answers identically
    clone = pickle.loads(pickle.dumps(model))
    clone.set_hyperparameters(11)
    np.testing.assert_array_equal(clone.predict(Xc)[0], mean)
    # d = 1, m = 1, default kernel, free noise
    X1 = rng.uniform(size=(15, 1))
    Y1 = [np.sin(5 * X1) + 0.05 * rng.normal(size=(15, 1))]
    m1 = B.multi_outputGP(1, n_samples=2, fixed_hyps=False)
    m1.n_burnin, m1.subsample_interval, m1.leapfrog_steps, m1.step_size, m1.max_iters = 2, 1, 2, 0.02, 20
    np.random.seed(4)
    m1.updateModel(X1, Y1)
    assert m1.hmc_samples[0].shape == (2, 3)                       # variance, one lengthscale, free noise
    inst = m1._instances[1]
    r1 = R.MultiOutputGPRef("se", [inst[0][0]], [inst[0][1]], [inst[0][2]])
    r1.updateModel(X1, Y1)
    m1.set_hyperparameters(1)
    x1 = rng.uniform(size=(9, 1))
    np.testing.assert_allclose(m1.predict(x1)[0], r1.predict(x1)[0], rtol=1e-5, atol=1e-6)
    np.testing.assert_allclose(m1.predict(x1)[1], r1.predict(x1)[1], rtol=1e-4, atol=1e-9)


@pytest.mark.parametrize("kind,N,d,m", [("se", 37, 3, 3), ("rbf", 128, 16, 2), ("matern52", 100, 5, 4), ("matern32", 64, 1, 1), ("se", 150, 4, 2)])
def test_fused_inference_equals_two_call_path(B, probes, kind, N, d, m):
    """bocf_infer: one fused launch for N <= 128, d <= 16 against bocf_fit + bocf_lml_gradients (and the oracle); N = 150
    takes the two-call path inside bocf_infer."""
    rng = np.random.RandomState(N + d)
    X = rng.uniform(size=(N, d))
    Ys = [np.sin(3 * X.sum(1) + j)[:, None] + 0.05 * rng.normal(size=(N, 1)) for j in range(m)]
    cls = {"se": B.kern.SE, "rbf": B.kern.RBF, "matern52": B.kern.Matern52, "matern32": B.kern.Matern32}[kind]
    kern = [cls(d, variance=0.7 + 0.3 * j, lengthscale=rng.uniform(0.4, 1.5, size=d), ARD=True) for j in range(m)]
    model = B.multi_outputGP(m, kernel=kern, noise_var=[None] * m, fixed_hyps=False, n_samples=2)
    model._X, model._Y = X, Ys
    model._create_sampler_state()
    params = [o.expanded(d) for o in model._sampler_outputs]
    fused = model._infer(params)
    model.set_option("fused_infer", 0)
    plain = model._infer(params)
    model.set_option("fused_infer", 1)
    np.testing.assert_allclose(fused[0], plain[0], rtol=1e-12)
    for a, b in zip(fused[1:], plain[1:]):
        np.testing.assert_allclose(a, b, rtol=1e-9, atol=1e-9 * np.abs(b).max())
    for j, (v, ls, nz) in enumerate(params):
        fit = R.GPFit(kind, X, Ys[j], v, ls, nz)
        np.testing.assert_allclose(fused[0][j], fit.log_marginal, rtol=1e-9)
        dv, dl, dn = fit.lml_gradients()
        np.testing.assert_allclose(fused[1][j], dv, rtol=1e-6, atol=1e-8)
        np.testing.assert_allclose(fused[2][j], dl, rtol=1e-6, atol=1e-7 * max(1.0, np.abs(dl).max()))
        np.testing.assert_allclose(fused[3][j], dn, rtol=1e-6, atol=1e-6)
    # the jitter ladder inside the fused launch loop: same jitter, same numbers as the two-call path
    if N <= 128:
        model.set_option("test_diag_shift_1e12", int(2.5e-4 * 1e12))
        with_jitter = model._infer(params)
        model.set_option("fused_infer", 0)
        plain_jitter = model._infer(params)
        model.set_option("fused_infer", 1)
        model.set_option("test_diag_shift_1e12", 0)
        np.testing.assert_allclose(with_jitter[0], plain_jitter[0], rtol=1e-12)
        np.testing.assert_allclose(with_jitter[2], plain_jitter[2], rtol=1e-8, atol=1e-8 * np.abs(plain_jitter[2]).max())
        assert not np.allclose(with_jitter[0], fused[0])


def test_cholesky_schedules_agree(B):
    """The blocked Cholesky's schedules (classic right-looking, G panels per trailing update, lookahead on a second stream, the
    reserved-CU schedule with device-side dependencies, early inverse on or off, wave-level or tiled row solves, resident teams per
    panel group) give the same factor up to rounding; N = 3300 (26 panels: the pair schedules need an even count) reaches every code
    path, one output keeps it quick."""
    N, d = 3300, 5
    p = R.synthetic_problem(N, d, 1, 64, 8, 77, noise=1e-4)
    Ls, preds = [], []
    for opts in ({"aggregate": 1, "lookahead": 0}, {"aggregate": 2}, {"aggregate": 4}, {"aggregate": 3},
                 {"lookahead": 2}, {"lookahead": 2, "overlap_inverse": 0}, {"lookahead": 0, "overlap_inverse": 1}, {"merge_x3": 2},
                 {"trsm_wave": 0, "lookahead": 0}, {"team_fit": 1, "team_panels": 3}, {"team_fit": 1, "team_panels": 8},
                 {"team_hybrid": 0, "team_fit": 1, "team_panels": 5}, {"team_hybrid": 1}, {"team_hybrid": 2, "team_panels": 4}, {"team_stream": 0},
                 {"team_crit_load": 64}, {"team_whole_max": 12}, {"aggregate": 0}):
        model = B.multi_outputGP(1, kernel=[_kern(B, "rbf", d, 1.0, p["lengthscales"][0])], noise_var=[1e-4], fixed_hyps=True)
        for k, v in opts.items():
            model.set_option(k, v)
        model.incremental = False
        model.updateModel(p["X"], p["Y"])          # (the FIRST factorization of a context always runs the single-stream schedule)
        model.updateModel(p["X"], p["Y"])
        assert model.jitter[0] == 0.0
        ctx = model._context()
        assert ctx.stat("sched_timeouts") == 0
        if ctx.stat("cu_masks_ok") and opts.get("lookahead", -1) == 2:
            assert ctx.stat("last_schedule") == 2, (opts, ctx.stat("last_schedule"))
        Ls.append(model.get_factor(0)[0])
        preds.append(model.predict(p["Xc"]))
    for L, (mean, var) in zip(Ls[1:], preds[1:]):
        np.testing.assert_allclose(L, Ls[0], rtol=1e-7, atol=1e-10)
        np.testing.assert_allclose(mean, preds[0][0], rtol=1e-7, atol=1e-8)
        np.testing.assert_allclose(var, preds[0][1], rtol=1e-5, atol=1e-9)
    fit = R.GPFit("rbf", p["X"], p["Y"][0], 1.0, p["lengthscales"][0], 1e-4)
    rm, rv = fit.predict(p["Xc"])
    np.testing.assert_allclose(preds[-1][0][0], rm[:, 0], rtol=1e-5, atol=1e-6)
    np.testing.assert_allclose(preds[-1][1][0], rv[:, 0], rtol=1e-4, atol=1e-9)


@pytest.mark.parametrize("N", [200, 300, 700, 1024, 2500])
def test_variance_gemm_tilings_are_bit_identical(B, N):
    """256-row tiles (default for large batches when the padded N is a multiple of 256) against the 128-row kernel:
    the same per-128-row partial sums in the same order, so exactly the same variances and acquisition values."""
    d, m, C = 4, (3 if N < 2000 else 1), 4096 + 37
    p = R.synthetic_problem(N, d, m, C, 32, 900 + N, noise=1e-5)
    model = _model(B, "matern52", p["X"], p["Y"], p["variances"], p["lengthscales"], p["noise"])
    out = []
    for sw in (0, 258, -1):
        model.set_option("swizzle", sw)
        out.append(model.predict(p["Xc"]))
    for mean, var in out[1:]:
        np.testing.assert_array_equal(mean, out[0][0])
        np.testing.assert_array_equal(var, out[0][1])
    ref = R.MultiOutputGPRef("matern52", p["variances"], p["lengthscales"], p["noise"])
    ref.updateModel(p["X"], p["Y"])
    rm, rv = ref.predict(p["Xc"][:300])
    np.testing.assert_allclose(out[2][1][:, :300], rv, rtol=1e-4, atol=1e-8)
