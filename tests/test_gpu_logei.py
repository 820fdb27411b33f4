"""Log-space expected improvement on the device (bocf_acq_log_linear, bocf_acq_log_mc, multi_outputGP.acq_log_linear / acq_log_mc, maLogEI,
LogEI, uLogEI) against the NumPy restatement tests/logei_ref.py -- never against another device path alone.

Gates.  Closed form on a host-given posterior: 10 x the restatement's own worst error against mpmath (60 digits) on the same points,
relative to max(1, |value|) -- computed here, at run time; the mixtures add the roundings of the log-sum-exp, (L H + 2) eps.  Monte-Carlo
kernel alone on a host-given posterior: rtol 1e-11 on log alpha.  Through the model against the restatement on the oracle's posterior:
values rtol 1e-5, atol 1e-12 (a logarithm: the natural scale is 1); gradients (at most 40 candidates, none left out) rtol 1e-4, atol 1e-9
max(1, |g|max).  Against the existing forms: exp(log EI) within rtol 1e-12 of bocf_acq_linear wherever that exceeds 1e-280, and
0 < exp(log alpha_tau) - EI <= tau (ln 2 + 0.1)(1 + 1e-12) for bocf_acq_mc; a further test walks the incumbent up until EI reaches 1e-280, where
bocf_acq_linear's own rounding, (z^4 / 2) eps, is the bound."""
import functools
import os
import sys

import mpmath as mp
import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import constrained_ref as CR  # noqa: E402
import kg_ref as K  # noqa: E402
import logei_ref as LR  # noqa: E402

import bocf_amd as B  # noqa: E402
from bocf_amd import _ffi  # noqa: E402
from bocf_amd import utility_program as UP  # noqa: E402
from oracle import cpu_ref as R  # noqa: E402

pytestmark = pytest.mark.gpu

KERN = {"rbf": B.kern.RBF, "se": B.kern.SE, "matern52": B.kern.Matern52, "matern32": B.kern.Matern32}
KID = {"rbf": _ffi.KERN_RBF, "se": _ffi.KERN_SE, "matern52": _ffi.KERN_MATERN52, "matern32": _ffi.KERN_MATERN32}
UTIL = {"linear": _ffi.UTIL_LINEAR, "neg_sq_dist": _ffi.UTIL_NEG_SQ_DIST, "neg_sum_exp": _ffi.UTIL_NEG_SUM_EXP,
        "neg_exp_cos": _ffi.UTIL_NEG_EXP_COS, "rosenbrock": _ffi.UTIL_ROSENBROCK}
MIXED = ["se", "matern52", "rbf", "matern32"]           # one family per output
EPS = np.finfo(float).eps
NGRAD = 40
Z_POINTS = [8.0, 1.0, 0.0, -1.0, np.nextafter(-1.0, 0.0), np.nextafter(-1.0, -2.0), -5.0, -29.999, -30.0, -30.001, -38.0, -40.0, -1e3, -1e6, -2.0 ** 26, -1e9,
            -1e12]
VARIANCES = [1e-10, 1.0, 1e6]


@pytest.fixture(scope="module")
def ctx():
    c = _ffi.Context(0)
    yield c
    c.close()


def _set_posterior(ctx, mean, var, mu_train, H=1):
    lib, dp = _ffi.load(), _ffi.dptr
    mean, var, mu_train = _ffi.f64(np.atleast_2d(mean)), _ffi.f64(np.atleast_2d(var)), _ffi.f64(np.atleast_2d(mu_train))
    _ffi.check(lib.bocf_set_posterior(ctx.handle, mean.shape[0], mean.shape[1], mu_train.shape[1], dp(mean), dp(var), dp(mu_train)), "bocf_set_posterior")
    ctx.set_option("hyper_samples", H)


def _log_linear(h, thetas, prob, C, grad_d=None):
    lib, dp = _ffi.load(), _ffi.dptr
    th, pr = _ffi.f64(np.atleast_2d(thetas)), None if prob is None else _ffi.f64(prob)
    got, dgot = np.empty(C), None if grad_d is None else np.empty((C, grad_d))
    return lib.bocf_acq_log_linear(h, dp(th), dp(pr), th.shape[0], dp(got), dp(dgot)), got, dgot


def _log_mc(h, tau, util, params, thetas, prob, C, grad_d=None, kind=None):
    lib, dp = _ffi.load(), _ffi.dptr
    th, par, pr = _ffi.f64(np.atleast_2d(thetas)), None if params is None else _ffi.f64(params), None if prob is None else _ffi.f64(prob)
    got, dgot = np.empty(C), None if grad_d is None else np.empty((C, grad_d))
    rc = lib.bocf_acq_log_mc(h, float(tau), UTIL[util] if kind is None else kind, dp(par), 0 if par is None else par.size, dp(th), th.shape[1], dp(pr), th.shape[0],
                             dp(got), dp(dgot))
    return rc, got, dgot


def _exact_term(sigma, z):
    """log sigma + log h(z) of the doubles sigma and z, at 60 digits."""
    with mp.workdps(60):                                   # (set locally: the precision is global state of mpmath)
        s, z = mp.mpf(float(sigma)), mp.mpf(float(z))
        return mp.log(s) + mp.log(mp.exp(-z * z / 2) / mp.sqrt(2 * mp.pi) + z * mp.erfc(-z / mp.sqrt(2)) / 2)


@functools.lru_cache(maxsize=None)
def _walk():
    """The points of the closed-form walk -- (variance, best, sigma, z as the doubles both sides compute, the restatement's value, the exact
    value) -- and the restatement's worst error on them relative to max(1, |value|)."""
    rows, worst = [], 0.0
    for v in VARIANCES:
        sigma = np.sqrt(v)
        for z0 in Z_POINTS:
            best = -z0 * sigma
            z = (0.0 - best) / sigma
            ref = float(LR.log_linear([np.zeros((1, 1))], [np.full((1, 1), v)], [np.array([best])], np.ones((1, 1)), None)[0])
            exact = _exact_term(sigma, z)
            worst = max(worst, float(abs(ref - exact) / max(1, abs(exact))))
            rows.append((v, best, sigma, z, ref, float(exact)))
    return rows, worst


# ---- 1. the closed form on a host-given posterior --------------------------------------------------------------------------------------
@pytest.mark.parametrize("C", [1, 3, 256, 257])
def test_closed_form_walks_z_on_a_host_given_posterior(ctx, C):
    """m = 1, mean 0, variance in {1e-10, 1, 1e6}, theta = 1; mu_train sets best so that z walks the list.  Every candidate of a batch gets the
    same value, the restatement's, within 10 x the restatement's own worst error against mpmath, relative to max(1, |value|)."""
    rows, e_ref = _walk()
    gate = 10.0 * e_ref
    worst_ref, worst_exact = 0.0, 0.0
    try:
        for v, best, sigma, z, ref, exact in rows:
            _set_posterior(ctx, np.zeros((1, C)), np.full((1, C), v), np.array([[best]]))
            rc, got, _ = _log_linear(ctx.handle, [[1.0]], None, C)
            assert rc == 0, _ffi.load().bocf_last_error()
            assert np.all(np.isfinite(got)) and np.all(got == got[0]), (v, z, got[:4])
            worst_ref = max(worst_ref, abs(got[0] - ref) / max(1.0, abs(ref)))
            worst_exact = max(worst_exact, abs(got[0] - exact) / max(1.0, abs(exact)))
            assert abs(got[0] - ref) <= gate * max(1.0, abs(ref)), (v, z, got[0], ref, gate)
    finally:
        ctx.set_option("hyper_samples", 1)
    print("closed form C %d: restatement against mpmath %.3g, device against the restatement %.3g, device against mpmath %.3g (relative to max(1, |value|)); gate %.3g"
          % (C, e_ref, worst_ref, worst_exact, gate))


# ---- 2. the mixture ------------------------------------------------------------------------------------------------------------------------
def _mixture_inputs(L, H, seed):
    """m = 2 outputs, C = 37 candidates; the parameters scale theta so that the terms lie up to more than 1e3 apart in log (z from the bulk
    to about -50); for L > 1 one theta is 0 (sigma = 0) and one weight is 0: the -inf terms."""
    rng = np.random.RandomState(seed)
    m, C, N = 2, 37, 9
    mean, var = rng.uniform(-1, 1, size=(H * m, C)), rng.uniform(0.01, 0.5, size=(H * m, C))
    mu_train = rng.uniform(-1, 1, size=(H * m, N))
    mu_train[0::m, 0] = 30.0                                # a far incumbent on output 0, for the thetas with weight on it ...
    thetas = rng.uniform(0.2, 1.0, size=(L, m))
    thetas[::2, 0] *= 1e-3                                  # ... which every other parameter all but ignores
    prob = rng.dirichlet(np.ones(L))
    if L > 1:
        thetas[1] = 0.0
        prob[L - 1] = 0.0
        prob /= prob.sum()
    return mean, var, mu_train, thetas, prob


@pytest.mark.parametrize("H", [1, 2])
@pytest.mark.parametrize("L", [1, 2, 32])
def test_mixture_on_a_host_given_posterior(ctx, L, H):
    mean, var, mu_train, thetas, prob = _mixture_inputs(L, H, 10 * L + H)
    m = 2
    sl = [slice(g * m, (g + 1) * m) for g in range(H)]
    bests = [LR.incumbents(mu_train[s], thetas) for s in sl]
    gate = 10.0 * _walk()[1] + (L * H + 2) * EPS
    try:
        _set_posterior(ctx, mean, var, mu_train, H)
        for pr in (prob, None):
            ref = LR.log_linear([mean[s] for s in sl], [var[s] for s in sl], bests, thetas, pr)
            rc, got, _ = _log_linear(ctx.handle, thetas, pr, mean.shape[1])
            assert rc == 0, _ffi.load().bocf_last_error()
            err = np.abs(got - ref) / np.maximum(1.0, np.abs(ref))
            print("mixture L %d H %d %s: log alpha in [%.4g, %.4g], worst error %.3g (gate %.3g)" % (L, H, "prob" if pr is not None else "mean", ref.min(), ref.max(),
                                                                                                  err.max(), gate))
            assert np.all(np.isfinite(got)) and np.all(err <= gate)
        if L > 1:
            # the terms really are far apart, and the -inf terms carry nothing: the mixture without them is the same
            one = [LR.log_linear([mean[sl[0]]], [var[sl[0]]], [bests[0][l:l + 1]], thetas[l:l + 1], None) for l in (0, L - 1 if L > 2 else 0)]
            keep = np.array([l for l in range(L) if l != 1 and prob[l] > 0])
            assert L == 2 or np.abs(one[0] - one[1]).max() > 1e3
            rc, got2, _ = _log_linear(ctx.handle, thetas[keep], prob[keep], mean.shape[1])
            rc1, got1, _ = _log_linear(ctx.handle, thetas, prob, mean.shape[1])
            assert rc == 0 and rc1 == 0
            np.testing.assert_allclose(got2, got1, rtol=gate, atol=gate)
        # every term -inf: -inf, no NaN
        rc, got, _ = _log_linear(ctx.handle, np.zeros((L, m)), None, mean.shape[1])
        assert rc == 0 and np.all(got == -np.inf)
        W = np.random.RandomState(1).normal(size=(5, m))
        _ffi.check(_ffi.load().bocf_set_mc_samples(ctx.handle, _ffi.dptr(_ffi.f64(W)), 5), "bocf_set_mc_samples")
        rc, got, _ = _log_mc(ctx.handle, 1.0, "linear", None, thetas, np.zeros(L), mean.shape[1])
        assert rc == 0 and np.all(got == -np.inf)
    finally:
        ctx.set_option("hyper_samples", 1)


# ---- models ------------------------------------------------------------------------------------------------------------------------------
def _fixed_model(kinds, X, Y, var, ls, noise):
    d = X.shape[1]
    model = B.multi_outputGP(len(kinds), kernel=[KERN[k](d, variance=var[j], lengthscale=ls[j], ARD=True) for j, k in enumerate(kinds)],
                             noise_var=list(noise), fixed_hyps=True)
    model.updateModel(X, [y[:, None] for y in Y])
    return model


def _hyper_model(kinds, X, Y, var, ls, noise, H):
    """H hyper-samples resident on the device: sample h scales the variances by 1 + 0.1 h and the lengthscales by 1 - 0.05 h."""
    m = len(kinds)
    model = B.multi_outputGP(m, fixed_hyps=False, n_samples=H)
    model._X, model._Y = np.ascontiguousarray(X), [y[:, None].copy() for y in Y]
    model._kernel_ids = [KID[k] for k in kinds]
    model._instances = [[(var[j] * (1 + 0.1 * h), ls[j] * (1 - 0.05 * h), noise[j]) for j in range(m)] for h in range(H)]
    model._fit()
    return model


# ---- 4. (and 3., 9.) the plateau: N = 40, d = 2, an incumbent that is hard to beat --------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _plateau():
    """A fitted two-output model whose incumbent sits on a high ridge, and the uniform candidates for which the restatement -- on the oracle's
    posterior, no device -- says: z < -45 for every theta (closed-form EI underflows below z = -38.6), every Monte-Carlo sample of the
    composite utility more than 1 below its incumbent, and the candidates' log values, of both forms, separated by more than 4 x the value
    gate (so that their order is decided)."""
    rng = np.random.RandomState(40)
    d, m, N = 2, 2, 40
    X = rng.uniform(size=(N, d))
    Y = [6.0 * np.exp(-8.0 * ((X[:, 0] - 0.85) ** 2 + (X[:, 1] - 0.8) ** 2)) + np.sin(3 * X[:, 0]), 5.0 * X[:, 0] * X[:, 1] + np.cos(2 * X[:, 1])]
    var, ls, nz = np.array([4.0, 4.0]), np.full((m, d), 0.4), np.full(m, 1e-3)
    kinds = ["rbf", "rbf"]
    la = K.LookAhead.fit(kinds, X, Y, var, ls, nz)
    thetas, prob = np.array([[0.7, 0.3], [0.4, 0.6]]), np.array([0.4, 0.6])
    targets = np.array([[6.0, 4.0], [5.0, 5.0]])           # the parameters of the composite utility -|y - t|^2
    W = np.random.RandomState(41).normal(size=(25, m))
    tau = 1e-2
    Q = rng.uniform(size=(600, d)) * np.array([0.6, 1.0])  # away from the ridge
    mean, v = CR.posterior(la, Q)
    mu_train = CR.train_mean(la)
    best_lin, best_sq = LR.incumbents(mu_train, thetas), LR.incumbents(mu_train, targets, "neg_sq_dist")
    z = np.stack([(th.dot(mean) - b) / np.sqrt((th * th).dot(v)) for th, b in zip(thetas, best_lin)])
    y = mean[:, None, :] + np.sqrt(v)[:, None, :] * W.T[:, :, None]
    gap = np.stack([R.utility_eval("neg_sq_dist", t, y.reshape(m, -1)).reshape(25, -1).max(0) - b for t, b in zip(targets, best_sq)])
    flat = np.all(z < -45.0, 0) & np.all(gap < -1.0, 0)
    lin = LR.log_linear([mean], [v], [best_lin], thetas, prob)
    mc = LR.log_mc([mean], [v], [best_sq], W, targets, prob, "neg_sq_dist", None, tau)
    keep = []
    for i in np.flatnonzero(flat):                         # greedy: separated from every candidate kept so far, in both forms
        if all(abs(lin[i] - lin[k]) > 4 * (1e-5 * abs(lin[i]) + 1e-12) and abs(mc[i] - mc[k]) > 4 * (1e-5 * abs(mc[i]) + 1e-12) for k in keep):
            keep.append(i)
    keep = np.array(keep[:120])
    return dict(kinds=kinds, X=X, Y=Y, var=var, ls=ls, nz=nz, la=la, thetas=thetas, prob=prob, targets=targets, W=W, tau=tau, Q=Q[keep], n_flat=int(flat.sum()),
                best_lin=best_lin, best_sq=best_sq)


_PLATEAU_MODEL = {}


def _plateau_model():
    if "m" not in _PLATEAU_MODEL:
        p = _plateau()
        _PLATEAU_MODEL["m"] = _fixed_model(p["kinds"], p["X"], p["Y"], p["var"], p["ls"], p["nz"])
    return _PLATEAU_MODEL["m"]


def _plateau_refs(p, X, grad=False):
    post = CR.posterior(p["la"], X, grad=grad)
    g = ([post[2]], [post[3]]) if grad else (None, None)
    lin = LR.log_linear([post[0]], [post[1]], [p["best_lin"]], p["thetas"], p["prob"], *g)
    mc = LR.log_mc([post[0]], [post[1]], [p["best_sq"]], p["W"], p["targets"], p["prob"], "neg_sq_dist", None, p["tau"], *g)
    return lin, mc


def test_the_point_of_the_feature_where_ei_is_exactly_zero():
    p, model = _plateau(), _plateau_model()
    Q = p["Q"]
    assert p["n_flat"] >= 100 and len(Q) >= 64
    # the existing forms: exactly 0.0 for every candidate, and a zero gradient
    assert np.all(model.acq_linear(Q, _ffi.ACQ_EI, p["thetas"], p["prob"]) == 0.0)
    a, g = model.acq_linear_grad(Q[:NGRAD], _ffi.ACQ_EI, p["thetas"], p["prob"])
    assert np.all(a == 0.0) and np.all(g == 0.0)
    assert np.all(model.acq_mc(Q, _ffi.ACQ_EI, _ffi.UTIL_NEG_SQ_DIST, None, p["targets"], p["prob"], W=p["W"]) == 0.0)
    a, g = model.acq_mc_grad(Q[:NGRAD], _ffi.UTIL_NEG_SQ_DIST, None, p["targets"], p["prob"], W=p["W"])
    assert np.all(a == 0.0) and np.all(g == 0.0)
    # the new forms: finite, in the restatement's order, select_topk the restatement's argsort
    ref_lin, ref_mc = _plateau_refs(p, Q)
    for name, ref, call in (("log_linear", ref_lin, lambda X, **kw: model.acq_log_linear(X, p["thetas"], p["prob"], **kw)),
                            ("log_mc", ref_mc, lambda X, **kw: model.acq_log_mc(X, _ffi.UTIL_NEG_SQ_DIST, None, p["targets"], p["prob"], p["tau"], W=p["W"], **kw))):
        got = call(Q)
        err = np.abs(got - ref)
        print("plateau %s: %d candidates, log alpha in [%.5g, %.5g], max err / (1e-5 |v| + 1e-12) %.3g" % (name, len(Q), ref.min(), ref.max(),
                                                                                                        np.max(err / (1e-5 * np.abs(ref) + 1e-12))))
        assert np.all(np.isfinite(got)) and np.all(err <= 1e-5 * np.abs(ref) + 1e-12)
        np.testing.assert_array_equal(np.argsort(-got, kind="stable"), np.argsort(-ref, kind="stable"))
        np.testing.assert_array_equal(model.select_topk(16)[0], np.argsort(-ref, kind="stable")[:16])
        np.testing.assert_array_equal(call(Q), got)                                 # a second identical call: the same bits
        refg = _plateau_refs(p, Q[:NGRAD], grad=True)[0 if name == "log_linear" else 1]
        v, dv = call(Q[:NGRAD], grad=True)
        print("plateau %s gradient: scale %.3g, max abs err %.3g" % (name, np.abs(refg[1]).max(), np.abs(dv - refg[1]).max()))
        assert np.all(np.isfinite(dv)) and np.all(np.abs(dv).max(1) > 0)
        assert np.all(np.abs(v - refg[0]) <= 1e-5 * np.abs(refg[0]) + 1e-12)
        np.testing.assert_allclose(dv, refg[1], rtol=1e-4, atol=1e-9 * max(1.0, np.abs(refg[1]).max()))
    # every term -inf (theta = 0: sigma = 0; every weight 0): the value is -inf and the gradient 0, never NaN
    v, dv = model.acq_log_linear(Q[:5], np.zeros((2, 2)), None, grad=True)
    assert np.all(v == -np.inf) and np.all(dv == 0.0)
    v, dv = model.acq_log_mc(Q[:5], _ffi.UTIL_NEG_SQ_DIST, None, p["targets"], np.zeros(2), p["tau"], W=p["W"], grad=True)
    assert np.all(v == -np.inf) and np.all(dv == 0.0)


def test_a_candidates_bits_do_not_depend_on_its_batch(ctx):
    rng = np.random.RandomState(8)
    m, C, S = 4, 261, 65
    mean, var, mu_train = rng.uniform(-1, 1, size=(m, C)), rng.uniform(0.01, 0.5, size=(m, C)), rng.uniform(-1, 1, size=(m, 7))
    thetas, prob, W = rng.uniform(-0.5, 0.5, size=(3, m)), rng.dirichlet(np.ones(3)), rng.normal(size=(S, m))
    lib, h = _ffi.load(), ctx.handle
    try:
        full = []
        for lo, hi in ((0, C), (3, 8), (255, 258), (260, 261)):
            _set_posterior(ctx, mean[:, lo:hi], var[:, lo:hi], mu_train)
            _ffi.check(lib.bocf_set_mc_samples(h, _ffi.dptr(_ffi.f64(W)), S), "bocf_set_mc_samples")
            a, b = _log_linear(h, thetas, prob, hi - lo), _log_mc(h, 1e-2, "neg_sq_dist", None, thetas, prob, hi - lo)
            assert a[0] == 0 and b[0] == 0
            if not full:
                full = [a[1], b[1]]
            np.testing.assert_array_equal(a[1], full[0][lo:hi])
            np.testing.assert_array_equal(b[1], full[1][lo:hi])
    finally:
        ctx.set_option("hyper_samples", 1)


# ---- 3. agreement with the existing forms ---------------------------------------------------------------------------------------------
def _ei_and_log_ei(ctx, seed, shift, m=3, C=257):
    """bocf_acq_linear's EI and bocf_acq_log_linear's log EI on one host-given posterior (both read the same arrays), with the smallest z of
    every candidate; `shift` raises the incumbent."""
    lib, dp, h = _ffi.load(), _ffi.dptr, ctx.handle
    rng = np.random.RandomState(seed)
    mean, var, mu_train = rng.uniform(-1, 1, size=(m, C)), rng.uniform(0.01, 0.5, size=(m, C)), rng.uniform(-1, 1, size=(m, 20)) + shift
    thetas, prob = rng.uniform(0.2, 1.0, size=(2, m)), np.array([0.3, 0.7])
    _set_posterior(ctx, mean, var, mu_train)
    ei = np.empty(C)
    _ffi.check(lib.bocf_acq_linear(h, _ffi.ACQ_EI, dp(_ffi.f64(thetas)), dp(prob), 2, dp(ei)), "bocf_acq_linear")
    rc, lg, _ = _log_linear(h, thetas, prob, C)
    assert rc == 0 and np.all(np.isfinite(lg))
    best = LR.incumbents(mu_train, thetas)
    zmin = np.min([(th.dot(mean) - b) / np.sqrt((th * th).dot(var)) for th, b in zip(thetas, best)], 0)
    ref = LR.log_linear([mean], [var], [best], thetas, prob)
    return ei, lg, zmin, ref


def test_agreement_with_the_existing_forms(ctx):
    """exp(bocf_acq_log_linear) against bocf_acq_linear at rtol 1e-12 wherever EI > 1e-280, on posteriors whose incumbent is the best of the
    training means (z from +3 down to about -10).  The Monte-Carlo form against bocf_acq_mc: 0 < exp(log alpha_tau) - EI <=
    tau (ln 2 + 0.1)(1 + 1e-12); the posterior is scaled with tau so that the surplus of a far sample, 0.1 tau^3 / (U - best)^2, stays above
    the rounding of EI itself."""
    lib, dp, h = _ffi.load(), _ffi.dptr, ctx.handle
    try:
        for seed in (0, 10, 20):
            ei, lg, zmin, _ = _ei_and_log_ei(ctx, seed, 0.0)
            ok = ei > 1e-280
            rel = np.abs(np.exp(lg[ok]) - ei[ok]) / ei[ok]
            print("seed %d: %d of %d candidates with EI > 1e-280, z from %.3g, worst relative difference %.3g" % (seed, ok.sum(), len(ei), zmin.min(), rel.max()))
            assert ok.sum() >= 250 and np.all(rel <= 1e-12)
        for util in ("linear", "neg_sq_dist"):
            for tau in (1e-6, 1e-2, 1.0):
                rng = np.random.RandomState(7)
                m, C, S, L = 4, 129, 30, 3
                scale = (np.sqrt(tau) if util == "neg_sq_dist" else tau) * 10.0
                mean, var, mu_train = scale * rng.uniform(-1, 1, size=(m, C)), scale ** 2 * rng.uniform(0.01, 0.5, size=(m, C)), scale * rng.uniform(-1, 1, size=(m, 15))
                thetas = rng.uniform(-0.5, 0.5, size=(L, m)) * (1.0 if util == "linear" else scale)
                W, prob = rng.normal(size=(S, m)), rng.dirichlet(np.ones(L))
                _set_posterior(ctx, mean, var, mu_train)
                _ffi.check(lib.bocf_set_mc_samples(h, dp(_ffi.f64(W)), S), "bocf_set_mc_samples")
                ei = np.empty(C)
                _ffi.check(lib.bocf_acq_mc(h, _ffi.ACQ_EI, UTIL[util], None, 0, dp(_ffi.f64(thetas)), m, dp(prob), L, dp(ei)), "bocf_acq_mc")
                rc, lg, _ = _log_mc(h, tau, util, None, thetas, prob, C)
                assert rc == 0 and np.all(np.isfinite(lg))
                diff = (np.exp(lg) - ei) / (tau * LR.BOUND)
                print("%s tau %g: EI in [%.3g, %.3g], surplus / (tau (ln 2 + 0.1)) in [%.3g, %.3g]" % (util, tau, ei.min(), ei.max(), diff.min(), diff.max()))
                assert np.all(diff > 0) and np.all(diff <= 1 + 1e-12)
    finally:
        ctx.set_option("hyper_samples", 1)


def test_in_the_tail_the_existing_closed_form_drifts_and_the_log_form_does_not(ctx):
    """Further cases, beyond the issue's: the incumbent raised until EI reaches down to 1e-280.  There bocf_acq_linear itself carries
    (z^4 / 2) eps = 2 (log EI)^2 eps relative (tests/test_logei_cpu.py has the derivation: 1e-12 at z = -11.6, 9e-11 at the far end), so
    exp(log EI) is held to that error of the existing form, times 4, plus 1e-12 -- while the log form stays within the closed-form gate of
    the restatement.  Measured on the MI355X: 2.1e-10 at worst, 0.41 of the bound."""
    gate = 10.0 * _walk()[1] + 4 * EPS
    try:
        n_tail = 0
        for seed, shift in ((1, 2.0), (2, 6.0), (3, 12.0)):
            ei, lg, zmin, ref = _ei_and_log_ei(ctx, seed, shift)
            assert np.all(np.abs(lg - ref) <= gate * np.maximum(1.0, np.abs(ref)))
            ok = ei > 1e-280
            n_tail += int(np.sum(ok & (zmin < -11.6)))
            le = np.abs(np.log(ei[ok]))
            rel = np.abs(np.exp(lg[ok]) - ei[ok]) / ei[ok]
            print("shift %g: %d candidates with EI > 1e-280, z from %.3g, worst relative difference %.3g, worst / (8 (log EI)^2 eps + 1e-12) %.3g"
                  % (shift, ok.sum(), zmin[ok].min(), rel.max(), np.max(rel / (8 * le * le * EPS + 1e-12))))
            assert np.all(rel <= 8 * le * le * EPS + 1e-12)
        assert n_tail >= 100
    finally:
        ctx.set_option("hyper_samples", 1)


# ---- 5. the Monte-Carlo kernels on a host-given posterior ---------------------------------------------------------------------------------
#        m  S   L  C    H  utility
KBASE = (4, 25, 4, 129, 1, "neg_sq_dist")


def _kvary(**kw):
    names = ("m", "S", "L", "C", "H", "util")
    c = dict(zip(names, KBASE))
    c.update(kw)
    return tuple(c[n] for n in names)


KERNEL = ([KBASE]
          + [_kvary(S=S, C=C) for S, C in ((1, 5), (2, 4), (63, 3), (64, 257), (65, 1), (130, 5), (1000, 3))]
          + [_kvary(m=mm, util=u) for mm in (1, 8, 9, 16) for u in ("neg_sq_dist", "linear")]
          + [_kvary(m=mm, util="rosenbrock") for mm in (4, 8, 16)]
          + [_kvary(L=1), _kvary(L=32, C=5), _kvary(H=2), _kvary(H=2, m=9, S=65, L=1)]
          + [_kvary(util=u, S=S, m=mm) for u in ("linear", "neg_sum_exp", "neg_exp_cos") for (S, mm) in ((25, 4), (130, 9))])
KIDS = ["m%d-S%d-L%d-C%d-H%d-%s" % c for c in KERNEL]


def _neg_sq_dist(t, y):
    return -np.sum(np.square((y.transpose() - t).transpose()), axis=0)


@pytest.mark.parametrize("case", KERNEL, ids=KIDS)
def test_monte_carlo_kernel_on_a_host_given_posterior(ctx, case):
    m, S, L, C, H, util = case
    rng = np.random.RandomState(500 + KERNEL.index(case))
    mean, var = rng.uniform(-1.0, 1.0, size=(H * m, C)), rng.uniform(0.01, 0.5, size=(H * m, C))
    mu_train = rng.uniform(-1.0, 1.0, size=(H * m, 11))
    W = rng.normal(size=(S, m))
    thetas, params = CR.utility_inputs(rng, util, m, L)
    prob = rng.dirichlet(np.ones(L))
    if L > 2:
        prob[1] = 0.0                                       # a -inf term
        prob /= prob.sum()
    sl = [slice(g * m, (g + 1) * m) for g in range(H)]
    lib, h, dp = _ffi.load(), ctx.handle, _ffi.dptr
    try:
        _set_posterior(ctx, mean, var, mu_train, H)
        _ffi.check(lib.bocf_set_mc_samples(h, dp(_ffi.f64(W)), S), "bocf_set_mc_samples")
        for bg in ((-1,) if H == 1 else (-1, 1)):
            ctx.set_option("best_group", bg)
            bests = [LR.incumbents(mu_train[sl[g if bg < 0 else bg]], thetas, util, params) for g in range(H)]
            for tau in (1e-3, 1.0):
                for pr in (prob, None):
                    ref = LR.log_mc([mean[s] for s in sl], [var[s] for s in sl], bests, W, thetas, pr, util, params, tau)
                    rc, got, _ = _log_mc(h, tau, util, params, thetas, pr, C)
                    assert rc == 0, lib.bocf_last_error()
                    err = np.abs(got - ref) / np.abs(ref)
                    print("kernel %s best_group %d tau %g %s: log alpha in [%.4g, %.4g], worst relative error %.3g" % (KIDS[KERNEL.index(case)], bg, tau,
                                                                                                              "prob" if pr is not None else "mean", ref.min(), ref.max(), err.max()))
                    assert np.all(np.isfinite(got)) and np.all(err <= 1e-11)
                    if util == "neg_sq_dist":
                        # the same expression traced as a utility program: against the restatement, like its compiled-in kind
                        blob = UP.trace(_neg_sq_dist, m, m).to_bytes()
                        _ffi.check(lib.bocf_set_utility_program(h, blob, len(blob)), "bocf_set_utility_program")
                        rc, gotp, _ = _log_mc(h, tau, util, None, thetas, pr, C, kind=_ffi.UTIL_PROGRAM)
                        assert rc == 0, lib.bocf_last_error()
                        assert np.all(np.abs(gotp - ref) <= 1e-11 * np.abs(ref))
        # the gradient form is refused by name on a host-given posterior
        rc, _, _ = _log_mc(h, 1.0, util, params, thetas, prob, C, grad_d=1)
        msg = lib.bocf_last_error()
        assert rc < 0 and b"bocf_acq_log_mc" in msg and b"host-given posterior" in msg
    finally:
        ctx.set_option("hyper_samples", 1)
        ctx.set_option("best_group", -1)


# ---- 6. through the model, against the restatement on the oracle's posterior ----------------------------------------------------------
#        N    d  m  H  utility
MODEL = [(40, 1, 1, 1, "linear"), (40, 6, 4, 2, "neg_sq_dist"), (130, 1, 4, 1, "neg_exp_cos"), (130, 6, 1, 2, "neg_sum_exp"), (130, 6, 4, 1, "rosenbrock"),
         (40, 6, 4, 2, "program")]
MIDS = ["N%d-d%d-m%d-H%d-%s" % c for c in MODEL]
_CACHE = {}


def _case(case):
    """(inputs, device model), made once per case; one case's model at a time."""
    if case not in _CACHE:
        N, d, m, H, util = case
        seed = 3000 + MODEL.index(case)
        kinds = [MIXED[j % 4] for j in range(m)]
        X, Y, var, ls, nz, Xc = K.problem(kinds, N, d, 129, seed, noise=1e-4)
        las = [K.LookAhead.fit(kinds, X, Y, var * (1 + 0.1 * h), ls * (1 - 0.05 * h), nz) for h in range(H)]
        rng = np.random.RandomState(7000 + seed)
        u = "neg_sq_dist" if util == "program" else util
        thetas, params = CR.utility_inputs(rng, u, m, 3)
        inp = dict(las=las, Xc=Xc, W=rng.normal(size=(25, m)), thetas=thetas, params=params, prob=rng.dirichlet(np.ones(3)), util=u, H=H, m=m,
                   lin_thetas=rng.uniform(0.2, 1.0, size=(3, m)), program=UP.trace(_neg_sq_dist, m, m).to_bytes() if util == "program" else None)
        a = (kinds, X, Y, var, ls, nz)
        _CACHE.clear()
        _CACHE[case] = (inp, _fixed_model(*a) if H == 1 else _hyper_model(*a, H))
    return _CACHE[case]


@pytest.mark.parametrize("case", MODEL, ids=MIDS)
def test_values_and_gradients_through_the_model(case):
    inp, model = _case(case)
    H, Xc, tau = inp["H"], inp["Xc"], 1e-2
    post = [CR.posterior(la, Xc) for la in inp["las"]]
    postg = [CR.posterior(la, Xc[:NGRAD], grad=True) for la in inp["las"]]
    mu_train = [CR.train_mean(la) for la in inp["las"]]
    kind = _ffi.UTIL_PROGRAM if inp["program"] else UTIL[inp["util"]]
    # the closed form: each hyper-sample's own incumbent, raised by nothing -- the bulk of z; the Monte-Carlo form: the incumbent of the
    # hyper-sample current on entry (the last)
    forms = [("log_linear", lambda g: LR.log_linear([p[0] for p in g], [p[1] for p in g], [LR.incumbents(mt, inp["lin_thetas"]) for mt in mu_train], inp["lin_thetas"],
                                                    inp["prob"], *(([p[2] for p in g], [p[3] for p in g]) if len(g[0]) > 2 else ())),
              lambda X, **kw: model.acq_log_linear(X, inp["lin_thetas"], inp["prob"], **kw)),
             ("log_mc", lambda g: LR.log_mc([p[0] for p in g], [p[1] for p in g], [LR.incumbents(mu_train[H - 1], inp["thetas"], inp["util"], inp["params"])] * H, inp["W"],
                                            inp["thetas"], inp["prob"], inp["util"], inp["params"], tau, *(([p[2] for p in g], [p[3] for p in g]) if len(g[0]) > 2 else ())),
              lambda X, **kw: model.acq_log_mc(X, kind, inp["params"], inp["thetas"], inp["prob"], tau, W=inp["W"], program=inp["program"], **kw))]
    for name, ref_of, call in forms:
        ref = ref_of(post)
        model.set_hyperparameters(H - 1)
        got = call(Xc)
        err = np.abs(got - ref)
        print("%s %s: log alpha in [%.4g, %.4g], max err / (1e-5 |v| + 1e-12) %.3g" % (MIDS[MODEL.index(case)], name, ref.min(), ref.max(),
                                                                                        np.max(err / (1e-5 * np.abs(ref) + 1e-12))))
        assert got.shape == (129,) and np.all(np.isfinite(got)) and np.all(err <= 1e-5 * np.abs(ref) + 1e-12)
        model.set_hyperparameters(H - 1)
        np.testing.assert_array_equal(call(Xc), got)
        rv, rg = ref_of(postg)
        model.set_hyperparameters(H - 1)
        v, dv = call(Xc[:NGRAD], grad=True)
        print("%s %s gradient: scale %.3g, max abs err %.3g" % (MIDS[MODEL.index(case)], name, np.abs(rg).max(), np.abs(dv - rg).max()))
        assert dv.shape == (NGRAD, Xc.shape[1]) and np.all(np.isfinite(dv)) and np.abs(rg).max() > 0
        assert np.all(np.abs(v - rv) <= 1e-5 * np.abs(rv) + 1e-12)
        np.testing.assert_allclose(dv, rg, rtol=1e-4, atol=1e-9 * max(1.0, np.abs(rg).max()))


# ---- 7. neutrality --------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", [MODEL[1], MODEL[4]], ids=[MIDS[1], MIDS[4]])
def test_the_improvement_acquisitions_return_the_same_bits_with_and_without_the_new_calls(case):
    inp, model = _case(case)
    H, Xc, m = inp["H"], inp["Xc"], inp["m"]
    rng = np.random.RandomState(1)
    kind = UTIL[inp["util"]]
    par = [(inp["thetas"], inp["prob"]), (inp["thetas"][::-1] * 0.9, inp["prob"][::-1].copy())]        # two parameter sets: a change in between
    lin = [(inp["lin_thetas"], inp["prob"]), (inp["lin_thetas"][:2] * 1.1, None)]

    def existing(i):
        model.set_hyperparameters(H - 1)
        a = model.acq_mc(Xc, _ffi.ACQ_EI, kind, inp["params"], par[i][0], par[i][1], W=inp["W"])
        model.set_hyperparameters(H - 1)
        b = model.acq_mc_grad(Xc[:NGRAD], kind, inp["params"], par[i][0], par[i][1], W=inp["W"])
        model.set_hyperparameters(H - 1)
        c = model.acq_linear(Xc, _ffi.ACQ_EI, lin[i][0], lin[i][1])
        return a, b[0], b[1], c

    def new_calls():
        model.set_hyperparameters(H - 1)
        model.acq_log_mc(Xc, kind, inp["params"], rng.permutation(par[0][0]) * 1.3, None, 0.5, W=inp["W"], grad=True)
        model.set_hyperparameters(H - 1)
        model.acq_log_linear(Xc, rng.uniform(0.1, 1.0, size=(4, m)), None, grad=True)
    plain = [existing(0), existing(1), existing(0)]
    mixed = []
    for i in (0, 1, 0):
        new_calls()
        a = model.set_hyperparameters(H - 1) or model.acq_mc(Xc, _ffi.ACQ_EI, kind, inp["params"], par[i][0], par[i][1], W=inp["W"])
        new_calls()
        model.set_hyperparameters(H - 1)
        b = model.acq_mc_grad(Xc[:NGRAD], kind, inp["params"], par[i][0], par[i][1], W=inp["W"])
        new_calls()
        model.set_hyperparameters(H - 1)
        c = model.acq_linear(Xc, _ffi.ACQ_EI, lin[i][0], lin[i][1])
        mixed.append((a, b[0], b[1], c))
    assert np.abs(plain[0][0]).max() > 0 and np.abs(plain[0][3]).max() > 0
    for p_, m_ in zip(plain, mixed):
        for x, y in zip(p_, m_):
            np.testing.assert_array_equal(x, y)


# ---- 8. refusals ----------------------------------------------------------------------------------------------------------------------------
def test_every_refusal_names_its_entry_point(ctx):
    lib, dp = _ffi.load(), _ffi.dptr
    th, out = np.zeros((2, 3)), np.empty(20)

    def bad(rc, name, text):
        msg = lib.bocf_last_error()
        assert rc < 0 and name.encode() in msg and text.encode() in msg, (rc, msg, text)
    fresh = _ffi.Context(0)
    bad(lib.bocf_acq_log_mc(fresh.handle, 1.0, 1, None, 0, dp(th), 3, None, 2, dp(out), None), "bocf_acq_log_mc", "model not fitted")
    bad(lib.bocf_acq_log_linear(fresh.handle, dp(th), None, 2, dp(out), None), "bocf_acq_log_linear", "model not fitted")
    fresh.close()
    kinds = MIXED[:3]
    X, Y, var, ls, nz, Xc = K.problem(kinds, 50, 2, 20, 9, noise=1e-4)
    model = _fixed_model(kinds, X, Y, var, ls, nz)
    model._ensure_fitted()
    h = model._context().handle
    assert lib.bocf_set_candidates(h, dp(_ffi.f64(Xc)), 20) == 0

    def mc(tau=1.0, util=_ffi.UTIL_NEG_SQ_DIST, theta=th, tdim=3, L=2, g=None):
        return lib.bocf_acq_log_mc(h, tau, util, None, 0, dp(theta), tdim, None, L, dp(out), dp(g))
    who = "bocf_acq_log_mc"
    bad(mc(), who, "no Monte-Carlo samples")
    model.set_mc_samples(np.random.RandomState(2).normal(size=(4, 3)))
    for tau in (0.0, -1.0, np.inf, np.nan):
        bad(mc(tau=tau), who, "tau must be finite and > 0")
    for L in (0, 33):
        bad(mc(L=L), who, "L out of range")
        bad(lib.bocf_acq_log_linear(h, dp(th), None, L, dp(out), None), "bocf_acq_log_linear", "L out of range")
    bad(mc(util=7), who, "unknown utility kind")
    bad(mc(theta=None), who, "theta")
    bad(mc(tdim=2), who, "theta_dim must equal m")
    bad(mc(util=_ffi.UTIL_PROGRAM), who, "no utility program is resident")
    blob = UP.trace(_neg_sq_dist, 2, 2).to_bytes()
    model.set_utility_program(blob)
    bad(mc(util=_ffi.UTIL_PROGRAM), who, "built for m = 2")
    blob = UP.trace(lambda t, y: y[0] * t[0], 3, 1).to_bytes()
    model.set_utility_program(blob)
    bad(mc(util=_ffi.UTIL_PROGRAM), who, "built for theta_dim = 1")
    assert mc(util=_ffi.UTIL_PROGRAM, tdim=1) == 0
    bad(lib.bocf_acq_log_linear(h, None, None, 2, dp(out), None), "bocf_acq_log_linear", "theta is null")
    assert lib.bocf_set_candidates(h, dp(_ffi.f64(Xc)), 0) == 0
    bad(mc(), who, "no resident candidates")
    bad(lib.bocf_acq_log_linear(h, dp(th), None, 2, dp(out), None), "bocf_acq_log_linear", "no resident candidates")
    assert lib.bocf_set_candidates(h, dp(_ffi.f64(Xc)), 20) == 0
    assert mc() == 0 and mc(g=np.empty((20, 2))) == 0
    assert lib.bocf_acq_log_linear(h, dp(th + 0.5), None, 2, dp(out), dp(np.empty((20, 2)))) == 0
    with pytest.raises(ValueError, match="output_dim"):
        model.acq_log_linear(Xc, np.zeros((1, 2)), None)
    # a gradient on a host-given posterior
    try:
        _set_posterior(ctx, np.zeros((3, 20)), np.ones((3, 20)), np.zeros((3, 1)))
        _ffi.check(lib.bocf_set_mc_samples(ctx.handle, dp(_ffi.f64(np.zeros((4, 3)))), 4), "bocf_set_mc_samples")
        bad(lib.bocf_acq_log_mc(ctx.handle, 1.0, 1, None, 0, dp(th), 3, None, 2, dp(out), dp(np.empty((20, 1)))), who, "host-given posterior")
        bad(lib.bocf_acq_log_linear(ctx.handle, dp(th), None, 2, dp(out), dp(np.empty((20, 1)))), "bocf_acq_log_linear", "host-given posterior")
    finally:
        ctx.set_option("hyper_samples", 1)


# ---- 9. the optimiser -------------------------------------------------------------------------------------------------------------------------
def test_the_classes_through_the_acquisition_optimizer_on_the_plateau():
    """optimize() of uLogEI and maLogEI on the N = 40 problem, where uEI and maEI are an exact zero over most of the box: the returned point's
    restatement value is at least that of the best start, within the through-model value gate (the optimiser saw the device's posterior,
    the restatement reads the oracle's)."""
    p, model = _plateau(), _plateau_model()
    space = B.Design_space([{'name': 'x', 'type': 'continuous', 'domain': (0, 1), 'dimensionality': 2}])
    dist = lambda s: B.ParameterDistribution(support=s, prob_dist=p["prob"])
    np.random.seed(5)
    cases = (("uLogEI", B.uLogEI, dict(utility=B.Utility(parameter_dist=dist(p["targets"]), device="neg_sq_dist"), tau=p["tau"]), 1),
             ("maLogEI", B.maLogEI, dict(utility=B.Utility(parameter_dist=dist(p["thetas"]), linear=True)), 0))
    for name, cls, kw, which in cases:
        opt = B.AcquisitionOptimizer(space, optimizer='lbfgs', n_starting=200, n_anchor=16)
        acq = cls(model, space, optimizer=opt, **kw)
        if which == 1:
            acq.W_samples = p["W"]
        x, fx = acq.optimize()
        anchors = opt.last_info["anchor_points"]
        assert x.shape == (1, 2) and np.all(x >= 0.0) and np.all(x <= 1.0) and len(anchors) == 16
        at_x, at_anchors = _plateau_refs(p, x)[which][0], _plateau_refs(p, anchors)[which]
        print("%s: restatement value at the optimum %.6g, at its 16 starts at best %.6g" % (name, at_x, at_anchors.max()))
        assert np.isfinite(at_x) and np.isfinite(float(np.squeeze(fx)))
        assert abs(-float(np.squeeze(fx)) - at_x) <= 1e-5 * abs(at_x) + 1e-12
        assert at_x >= at_anchors.max() - (1e-5 * abs(at_anchors.max()) + 1e-12)
        with pytest.raises(NotImplementedError, match="refine='device' does not cover %s" % name):
            cls(model, space, optimizer=B.AcquisitionOptimizer(space, optimizer='lbfgs', n_starting=50, n_anchor=4, refine="device"), **kw).optimize()
    # one iteration of the outer loop, unchanged: Sequential and CBO take the new class as they take any other
    f = [lambda x: np.sin(3 * x[:, :1]) * x[:, 1:2], lambda x: np.cos(2 * x[:, 1:2]) + 0.5 * x[:, :1]]
    m2 = _fixed_model(p["kinds"], p["X"], p["Y"], p["var"], p["ls"], p["nz"])
    acq = B.uLogEI(m2, space, optimizer=B.AcquisitionOptimizer(space, optimizer='lbfgs', n_starting=100, n_anchor=8), tau=p["tau"],
                   utility=B.Utility(parameter_dist=dist(p["targets"]), device="neg_sq_dist"))
    bo = B.CBO(m2, space, B.MultiObjective(f, noise_var=[1e-3, 1e-3]), acq, B.Sequential(acq), p["X"])
    bo.run_optimization(max_iter=1)
    assert bo.X.shape == (41, 2) and np.all(bo.X >= 0.0) and np.all(bo.X <= 1.0)
