"""Quantile / tail-mean acquisitions of the composite utility and the closed-form confidence bound on the device (bocf_acq_risk,
bocf_acq_linear_ucb, multi_outputGP.acq_risk / acq_linear_ucb, uUCB, uCVaR, maUCB) against the NumPy restatement tests/risk_ref.py -- never
against another device path alone.

Gates.  Exact selection (a host-given posterior with mean 0 and variance 1, the linear utility with theta = 1, so u_s IS W_s): the quantile
with ==, the tail means within rtol 1e-13 of math.fsum over the restatement's tail.  Kernel alone on a host-given posterior: rtol 1e-11,
atol 1e-14 max_s |u_s| of the candidate -- an order statistic moves by at most the largest perturbation of any one sample, so the absolute
part scales with the largest sample, not with the result.  Through the model against the restatement on the oracle's posterior: values rtol
1e-5, atol 1e-12 max_s |u_s|; gradients (at most 40 candidates) rtol 1e-4, atol 1e-9 max(1, |g|max), compared only for the candidates
whose u_(k) is further than 1e-6 max_s |u_s| from both neighbours in the order for every theta and hyper-sample (below that, which sample
is selected is undecided between the device's and NumPy's rounding); at most 5 % of the candidates may be left out that way."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import constrained_ref as CR  # noqa: E402
import kg_ref as K  # noqa: E402
import risk_ref as RR  # noqa: E402

import bocf_amd as B  # noqa: E402
from bocf_amd import _ffi  # noqa: E402

pytestmark = pytest.mark.gpu

KERN = {"rbf": B.kern.RBF, "se": B.kern.SE, "matern52": B.kern.Matern52, "matern32": B.kern.Matern32}
KID = {"rbf": _ffi.KERN_RBF, "se": _ffi.KERN_SE, "matern52": _ffi.KERN_MATERN52, "matern32": _ffi.KERN_MATERN32}
UTIL = {"linear": _ffi.UTIL_LINEAR, "neg_sq_dist": _ffi.UTIL_NEG_SQ_DIST, "neg_sum_exp": _ffi.UTIL_NEG_SUM_EXP,
        "neg_exp_cos": _ffi.UTIL_NEG_EXP_COS, "rosenbrock": _ffi.UTIL_ROSENBROCK}
MIXED = ["se", "matern52", "rbf", "matern32"]           # one family per output
KINDS = [RR.QUANTILE, RR.UPPER_TAIL, RR.LOWER_TAIL]
KIND_NAMES = {RR.QUANTILE: "quantile", RR.UPPER_TAIL: "upper", RR.LOWER_TAIL: "lower"}
NGRAD = 40


@pytest.fixture(scope="module")
def ctx():
    c = _ffi.Context(0)
    yield c
    c.close()


def _risk_call(lib, h, kind, k, util, params, thetas, prob, C, grad_d=None):
    dp = _ffi.dptr
    th, par, pr = _ffi.f64(np.atleast_2d(thetas)), None if params is None else _ffi.f64(params), None if prob is None else _ffi.f64(prob)
    got = np.empty(C)
    dgot = None if grad_d is None else np.empty((C, grad_d))
    rc = lib.bocf_acq_risk(h, kind, k, UTIL[util], dp(par), 0 if par is None else par.size, dp(th), th.shape[1], dp(pr), th.shape[0], dp(got), dp(dgot))
    return rc, got, dgot


# ---- exact selection: the test that pins the kernel ------------------------------------------------------------------------------------
SIZES = [1, 2, 63, 64, 65, 127, 128, 130, 1000, 4096]
PATTERNS = ["permutation", "sorted", "reversed", "all_equal", "duplicate_blocks", "last_bit", "tiny_mixed", "infinities"]


def _pattern(name, S, rng):
    """S doubles; no -0.0 among them (every pattern is compared as numbers anyway)."""
    if name == "permutation":
        return rng.permutation(S).astype(float) - S // 3
    if name == "sorted":
        return np.sort(rng.normal(size=S))
    if name == "reversed":
        return np.sort(rng.normal(size=S))[::-1].copy()
    if name == "all_equal":
        return np.full(S, 0.3)
    if name == "duplicate_blocks":
        # runs of 5 equal values, one long run over the middle half (it straddles S // 2), shuffled: every rank asked for lies in a run
        v = (np.arange(S) // 5).astype(float)
        v[S // 4:3 * S // 4 + 1] = v[S // 2]
        return rng.permutation(v)
    if name == "last_bit":
        return rng.permutation(1.0 + np.arange(S) * np.finfo(float).eps)
    if name == "tiny_mixed":
        mag = np.array([5e-324, 1.2e-320, 2.2250738585072014e-308, 1e-300, 1e-200, 1e-30, 1e-5, 1.0, 3.0])
        v = rng.choice(mag, size=S) * rng.choice([-1.0, 1.0], size=S) * rng.uniform(1.0, 2.0, size=S)
        return np.where(v == 0.0, 5e-324, v)
    v = rng.normal(size=S)
    v[rng.permutation(S)[:max(1, S // 8)]] = np.inf
    if S > 1:
        v[rng.permutation(S)[:max(1, S // 9)]] = -np.inf
    return v


@pytest.mark.parametrize("pattern", PATTERNS)
@pytest.mark.parametrize("S", SIZES)
def test_exact_selection(ctx, S, pattern):
    lib, h, dp = _ffi.load(), ctx.handle, _ffi.dptr
    rng = np.random.RandomState(1000 * PATTERNS.index(pattern) + S)
    W = _pattern(pattern, S, rng)
    assert W.shape == (S,) and not np.any(np.signbit(W) & (W == 0.0))
    srt = np.sort(W)
    ranks = sorted({k for k in (0, 1, S // 2, S - 2, S - 1) if 0 <= k < S})
    want = {}
    for k in ranks:
        want[(RR.QUANTILE, k)] = srt[k]
        want[(RR.UPPER_TAIL, k)] = RR.tail_mean(srt[k:])
        want[(RR.LOWER_TAIL, k)] = RR.tail_mean(srt[:k + 1])
        for kind in KINDS:                                           # (the restatement's own order gives the same sets)
            rho = RR.statistic(W, kind, k)[0]
            assert rho == want[(kind, k)] or (np.isnan(rho) and np.isnan(want[(kind, k)]))
    worst = 0.0
    for C in (1, 3, 4, 5, 257):
        _ffi.check(lib.bocf_set_posterior(h, 1, C, 1, dp(np.zeros((1, C))), dp(np.ones((1, C))), dp(np.zeros((1, 1)))), "bocf_set_posterior")
        _ffi.check(lib.bocf_set_mc_samples(h, dp(_ffi.f64(W[:, None])), S), "bocf_set_mc_samples")
        for k in ranks:
            for kind in KINDS:
                rc, got, _ = _risk_call(lib, h, kind, k, "linear", None, [[1.0]], None, C)
                assert rc == 0, lib.bocf_last_error()
                w = want[(kind, k)]
                if kind == RR.QUANTILE:
                    assert np.all(got == w), (S, pattern, C, k, got[:4], w)
                else:
                    if np.isfinite(w) and w != 0.0:
                        worst = max(worst, np.abs(got - w).max() / abs(w))
                    np.testing.assert_allclose(got, np.full(C, w), rtol=1e-13, atol=0, err_msg="S %d %s C %d k %d %s" % (S, pattern, C, k, KIND_NAMES[kind]))
    print("exact selection S %d %s: %d ranks x 3 kinds x 5 batch sizes, worst relative tail-mean error %.3g" % (S, pattern, len(ranks), worst))


def test_a_nan_utility_ranks_and_counts_as_minus_infinity(ctx):
    lib, h, dp = _ffi.load(), ctx.handle, _ffi.dptr
    rng = np.random.RandomState(5)
    m, C, S = 2, 6, 25
    mean, var, W = rng.uniform(-1, 1, size=(m, C)), rng.uniform(0.01, 0.5, size=(m, C)), rng.normal(size=(S, m))
    mean[0, 2] = np.nan
    _ffi.check(lib.bocf_set_posterior(h, m, C, 1, dp(_ffi.f64(mean)), dp(_ffi.f64(var)), dp(np.zeros((m, 1)))), "bocf_set_posterior")
    _ffi.check(lib.bocf_set_mc_samples(h, dp(_ffi.f64(W)), S), "bocf_set_mc_samples")
    for kind in KINDS:
        for k in (0, 12, 24):
            ref = RR.risk(mean, var, W, np.zeros((1, 1)), None, "neg_sum_exp", None, kind, k)
            rc, got, _ = _risk_call(lib, h, kind, k, "neg_sum_exp", None, np.zeros((1, 1)), None, C)
            assert rc == 0, lib.bocf_last_error()
            assert got[2] == -np.inf == ref["alpha"][2]
            ok = np.arange(C) != 2
            assert np.all(np.isfinite(got[ok]))
            assert np.all(np.abs(got[ok] - ref["alpha"][ok]) <= 1e-11 * np.abs(ref["alpha"][ok]) + 1e-14 * ref["scale"][ok])


# ---- the kernels alone, on a host-given posterior ----------------------------------------------------------------------------------------
#        m  S   L  C    H  utility        prob
CBASE = (4, 25, 3, 129, 1, "neg_sq_dist", True)


def _cvary(**kw):
    names = ("m", "S", "L", "C", "H", "util", "prob")
    c = dict(zip(names, CBASE))
    c.update(kw)
    return tuple(c[n] for n in names)


CANNED = ([CBASE]
          + [_cvary(m=1), _cvary(m=2, util="rosenbrock"), _cvary(m=4, util="rosenbrock"), _cvary(m=8), _cvary(m=8, util="rosenbrock"), _cvary(m=9),
             _cvary(m=16), _cvary(m=16, util="rosenbrock")]
          + [_cvary(L=1, prob=False), _cvary(L=1), _cvary(L=3, prob=False)]
          + [_cvary(S=64), _cvary(S=130), _cvary(S=130, m=9)]
          + [_cvary(H=2)]
          + [_cvary(util=u, S=S, m=m) for u in ("linear", "neg_sum_exp", "neg_exp_cos") for (S, m) in ((25, 4), (64, 2), (130, 9))])
CIDS = ["m%d-S%d-L%d-C%d-H%d-%s-%s" % (c[:6] + ("prob" if c[6] else "mean",)) for c in CANNED]


@pytest.mark.parametrize("case", CANNED, ids=CIDS)
def test_kernel_on_a_canned_posterior(ctx, case):
    m, S, L, C, H, util, with_prob = case
    rng = np.random.RandomState(300 + CANNED.index(case))
    mean, var = rng.uniform(-1.0, 1.0, size=(H * m, C)), rng.uniform(0.01, 0.5, size=(H * m, C))
    W = rng.normal(size=(S, m))
    thetas, params = CR.utility_inputs(rng, util, m, L)
    prob = rng.dirichlet(np.ones(L)) if with_prob else None
    sl = [slice(g * m, (g + 1) * m) for g in range(H)]
    lib, h, dp = _ffi.load(), ctx.handle, _ffi.dptr
    _ffi.check(lib.bocf_set_posterior(h, H * m, C, 1, dp(_ffi.f64(mean)), dp(_ffi.f64(var)), dp(np.zeros((H * m, 1)))), "bocf_set_posterior")
    ctx.set_option("hyper_samples", H)
    try:
        _ffi.check(lib.bocf_set_mc_samples(h, dp(_ffi.f64(W)), S), "bocf_set_mc_samples")
        for kind in KINDS:
            for k in sorted({0, S // 2, RR.rank_of(0.9, S), S - 1}):
                ref = RR.risk_hyper([mean[s] for s in sl], [var[s] for s in sl], W, thetas, prob, util, params, kind, k)
                rc, got, _ = _risk_call(lib, h, kind, k, util, params, thetas, prob, C)
                assert rc == 0, lib.bocf_last_error()
                err = np.abs(got - ref["alpha"])
                print("canned %s %s k %d: max |alpha| %.3g, max abs err %.3g, max err / (1e-11 |alpha| + 1e-14 scale) %.3g"
                      % (CIDS[CANNED.index(case)], KIND_NAMES[kind], k, np.abs(ref["alpha"]).max(), err.max(),
                         np.max(err / (1e-11 * np.abs(ref["alpha"]) + 1e-14 * ref["scale"]))))
                assert np.all(np.isfinite(got))
                assert np.all(err <= 1e-11 * np.abs(ref["alpha"]) + 1e-14 * ref["scale"])
        # the gradient form is refused by name on a host-given posterior
        rc, _, _ = _risk_call(lib, h, RR.QUANTILE, 0, util, params, thetas, prob, C, grad_d=1)
        msg = lib.bocf_last_error()
        assert rc < 0 and b"bocf_acq_risk" in msg and b"host-given posterior" in msg
    finally:
        ctx.set_option("hyper_samples", 1)


def test_selection_after_the_call_is_the_restatements_stable_argsort(ctx):
    rng = np.random.RandomState(17)
    m, C, S = 4, 129, 25
    mean, var = rng.uniform(-1, 1, size=(m, C)), rng.uniform(0.01, 0.5, size=(m, C))
    W, thetas = rng.normal(size=(S, m)), rng.uniform(-0.5, 0.5, size=(3, m))
    ref = RR.risk(mean, var, W, thetas, None, "neg_sq_dist", None, RR.QUANTILE, 22)
    full = np.argsort(-ref["alpha"], kind="stable")
    top = ref["alpha"][full[:17]]
    assert np.all(top[:-1] - top[1:] > 1e-9 * ref["scale"].max())   # the first 16 are separated by far more than the kernel's error
    lib, h, dp = _ffi.load(), ctx.handle, _ffi.dptr
    _ffi.check(lib.bocf_set_posterior(h, m, C, 1, dp(_ffi.f64(mean)), dp(_ffi.f64(var)), dp(np.zeros((m, 1)))), "bocf_set_posterior")
    _ffi.check(lib.bocf_set_mc_samples(h, dp(_ffi.f64(W)), S), "bocf_set_mc_samples")
    _ffi.check(lib.bocf_acq_risk(h, RR.QUANTILE, 22, _ffi.UTIL_NEG_SQ_DIST, None, 0, dp(_ffi.f64(thetas)), m, None, 3, None, None), "bocf_acq_risk")
    idx, val = np.empty(16, dtype=np.int64), np.empty(16)
    _ffi.check(lib.bocf_select_topk(h, 16, idx.ctypes.data_as(_ffi._c_ll_p), dp(val)), "bocf_select_topk")
    np.testing.assert_array_equal(idx, full[:16])
    np.testing.assert_allclose(val, ref["alpha"][full[:16]], rtol=1e-11, atol=1e-14 * ref["scale"].max())


# ---- through the model, against the restatement on the oracle's posterior ----------------------------------------------------------------
#        N    d  m  S   L  C    H  utility        prob
MBASE = (120, 3, 4, 25, 3, 129, 1, "neg_sq_dist", True)


def _mvary(**kw):
    names = ("N", "d", "m", "S", "L", "C", "H", "util", "prob")
    c = dict(zip(names, MBASE))
    c.update(kw)
    return tuple(c[n] for n in names)


MODEL = [MBASE, _mvary(N=64, d=1), _mvary(N=64, d=6, S=64), _mvary(N=120, d=6, util="neg_exp_cos", m=3), _mvary(N=64, d=3, H=2),
         _mvary(N=120, d=1, H=2, util="rosenbrock", m=2, S=130, L=1, prob=False)]
MIDS = ["N%d-d%d-m%d-S%d-L%d-C%d-H%d-%s-%s" % (c[:8] + ("prob" if c[8] else "mean",)) for c in MODEL]


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


def _inputs(case):
    N, d, m, S, L, C, H, util, with_prob = case
    seed = 2000 + MODEL.index(case)
    kinds = [MIXED[j % 4] for j in range(m)]
    X, Y, var, ls, nz, Xc = K.problem(kinds, N, d, C, seed, noise=1e-4)
    las = [K.LookAhead.fit(kinds, X, Y, var * (1 + 0.1 * h), ls * (1 - 0.05 * h), nz) for h in range(H)]
    rng = np.random.RandomState(7000 + seed)
    W = rng.normal(size=(S, m))
    thetas, params = CR.utility_inputs(rng, util, m, L)
    prob = rng.dirichlet(np.ones(L)) if with_prob else None
    return dict(kinds=kinds, X=X, Y=Y, var=var, ls=ls, nz=nz, Xc=Xc, las=las, W=W, thetas=thetas, params=params, prob=prob, util=util, H=H,
                k=RR.rank_of(0.9, S))


def _reference(inp, kind, grad):
    """The restatement on the oracle's posterior: all candidates (values), or the first NGRAD with gradients."""
    Xc = inp["Xc"][:NGRAD] if grad else inp["Xc"]
    post = [CR.posterior(la, Xc, grad=grad) for la in inp["las"]]
    return RR.risk_hyper([p[0] for p in post], [p[1] for p in post], inp["W"], inp["thetas"], inp["prob"], inp["util"], inp["params"], kind, inp["k"],
                         dmeans=[p[2] for p in post] if grad else None, dvars=[p[3] for p in post] if grad else None)


def compared_rows(ref):
    """Candidates whose gradient is compared: u_(k) further than 1e-6 max|u_s| from both neighbours, for every theta and hyper-sample."""
    return ref["gap"].min(1) > 1e-6 * ref["scale"]


_CACHE = {}


def _case(case):
    """(inputs, device model), made once per case."""
    if case not in _CACHE:
        inp = _inputs(case)
        a = (inp["kinds"], inp["X"], inp["Y"], inp["var"], inp["ls"], inp["nz"])
        model = _fixed_model(*a) if inp["H"] == 1 else _hyper_model(*a, inp["H"])
        _CACHE.clear()                                    # one case's model at a time
        _CACHE[case] = (inp, model)
    return _CACHE[case]


def _device(model, inp, X, kind, grad=False):
    model.set_hyperparameters(inp["H"] - 1)
    return model.acq_risk(X, kind, inp["k"], UTIL[inp["util"]], inp["params"], inp["thetas"], inp["prob"], W=inp["W"], grad=grad)


@pytest.mark.parametrize("kind", KINDS, ids=[KIND_NAMES[k] for k in KINDS])
@pytest.mark.parametrize("case", MODEL, ids=MIDS)
def test_values_and_gradients_against_the_restatement(case, kind):
    """Share of the 40 gradient candidates left out by the gap rule, from the restatement alone (the oracle's posterior, no device): 0 of 40 in
    every case and kind of MODEL with these seeds."""
    inp, model = _case(case)
    ref = _reference(inp, kind, False)
    got = _device(model, inp, inp["Xc"], kind)
    err = np.abs(got - ref["alpha"])
    print("risk %s %s: max |alpha| %.3g, max abs err %.3g, max err / (1e-5 |alpha| + 1e-12 scale) %.3g"
          % (MIDS[MODEL.index(case)], KIND_NAMES[kind], np.abs(ref["alpha"]).max(), err.max(), np.max(err / (1e-5 * np.abs(ref["alpha"]) + 1e-12 * ref["scale"]))))
    assert got.shape == (case[5],) and np.all(np.isfinite(got))
    assert np.all(err <= 1e-5 * np.abs(ref["alpha"]) + 1e-12 * ref["scale"])
    np.testing.assert_array_equal(_device(model, inp, inp["Xc"], kind), got)          # a second identical call: the same bits
    if inp["H"] > 1:
        # there is no incumbent: option best_group, unset or set, does not matter
        lib, h = _ffi.load(), model._context().handle
        for bg in (-1, 0, inp["H"] - 1):
            model._context().set_option("best_group", bg)
            rc, again, _ = _risk_call(lib, h, kind, inp["k"], inp["util"], inp["params"], inp["thetas"], inp["prob"], case[5])
            assert rc == 0, lib.bocf_last_error()
            np.testing.assert_array_equal(again, got)
    refg = _reference(inp, kind, True)
    X = inp["Xc"][:NGRAD]
    got, dgot = _device(model, inp, X, kind, grad=True)
    keep = compared_rows(refg)
    g = refg["dalpha"]
    print("risk gradient %s %s: %d of %d candidates compared, max abs err %.3g, gradient scale %.3g"
          % (MIDS[MODEL.index(case)], KIND_NAMES[kind], keep.sum(), len(X), np.abs(dgot - g)[keep].max(), np.abs(g).max()))
    assert dgot.shape == X.shape and np.all(np.isfinite(dgot))
    assert np.mean(~keep) <= 0.05
    assert np.all(np.abs(got - refg["alpha"]) <= 1e-5 * np.abs(refg["alpha"]) + 1e-12 * refg["scale"])
    assert np.abs(g[keep]).max() > 0
    np.testing.assert_allclose(dgot[keep], g[keep], rtol=1e-4, atol=1e-9 * max(1.0, np.abs(g).max()))


def test_device_gradient_against_central_differences_of_the_device_value():
    """At the candidate whose u_(k) is best separated (the selected sample is the same at x - h, x, x + h): the finite-difference gate of the
    other acquisitions, rtol 1e-3, atol 1e-6 max(1, |g|max)."""
    inp, model = _case(MBASE)
    for kind in KINDS:
        refg = _reference(inp, kind, True)
        i = int(np.argmax(refg["gap"].min(1) / refg["scale"]))
        assert refg["gap"][i].min() > 1e-3 * refg["scale"][i]
        x = inp["Xc"][i:i + 1]
        _, g = _device(model, inp, x, kind, grad=True)
        h, fd = 1e-6, np.zeros_like(x)
        for q in range(x.shape[1]):
            xp, xm = x.copy(), x.copy()
            xp[0, q] += h
            xm[0, q] -= h
            fd[0, q] = (_device(model, inp, xp, kind)[0] - _device(model, inp, xm, kind)[0]) / (2 * h)
        assert np.abs(g).max() > 0
        np.testing.assert_allclose(g, fd, rtol=1e-3, atol=1e-6 * max(1.0, np.abs(g).max()))


# ---- the closed form ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("L", [1, 3])
@pytest.mark.parametrize("kappa", [0.0, 2.0])
def test_linear_ucb_against_numpy(kappa, L):
    case = _mvary(N=64, d=3, H=2)
    inp, model = _case(case)
    rng = np.random.RandomState(11 + L)
    thetas = rng.uniform(-0.5, 0.5, size=(L, case[2]))
    prob = rng.dirichlet(np.ones(L)) if L > 1 else None
    post = [CR.posterior(la, inp["Xc"], grad=True) for la in inp["las"]]
    want = np.mean([RR.linear_ucb(p[0], p[1], thetas, prob, kappa) for p in post], 0)
    model.set_hyperparameters(inp["H"] - 1)
    got = model.acq_linear_ucb(inp["Xc"], kappa, thetas, prob)
    np.testing.assert_allclose(got, want, rtol=1e-5, atol=1e-12)
    X = inp["Xc"][:NGRAD]
    model.set_hyperparameters(inp["H"] - 1)
    got2, dgot = model.acq_linear_ucb(X, kappa, thetas, prob, grad=True)
    g = np.mean([RR.linear_ucb(p[0][:, :NGRAD], p[1][:, :NGRAD], thetas, prob, kappa, p[2][:, :NGRAD], p[3][:, :NGRAD])[1] for p in post], 0)
    np.testing.assert_allclose(got2, want[:NGRAD], rtol=1e-5, atol=1e-12)
    np.testing.assert_allclose(dgot, g, rtol=1e-4, atol=1e-9 * max(1.0, np.abs(g).max()))
    if kappa == 0.0:
        # the bound at kappa = 0 is theta^T mu of the DEVICE's own posterior mean, to rtol 1e-12 and nothing else, on the candidates where
        # that is well posed: the terms have both signs and the two sides add them in different orders, at most fifteen roundings of the
        # sum of their magnitudes each (m + 2 L + 2 H), so where that sum is within 100 |theta^T mu| the sides agree to 2 * 15 * 1.1e-16 * 100 = 3.3e-13.
        # On the oracle's posterior that holds for 127 of 129 candidates at L = 1 and for all at L = 3; at least 95 % are required here.
        p = np.full(L, 1.0 / L) if prob is None else prob
        mus, mags = [], []
        for hh in range(inp["H"]):
            model.set_hyperparameters(hh)
            mu = model.posterior_mean(inp["Xc"])
            mus.append(p.dot(thetas.dot(mu)))
            mags.append(p.dot(np.abs(thetas).dot(np.abs(mu))))
        want0 = np.mean(mus, 0)
        posed = np.mean(mags, 0) <= 100.0 * np.abs(want0)
        assert np.mean(posed) >= 0.95
        np.testing.assert_allclose(got[posed], want0[posed], rtol=1e-12, atol=0)


# ---- the classes ----------------------------------------------------------------------------------------------------------------------------
def _surface_problem(seed=41):
    np.random.seed(seed)
    d, m = 2, 2
    space = B.Design_space([{'name': 'x', 'type': 'continuous', 'domain': (0, 1), 'dimensionality': d}])
    f = [lambda x: np.sin(3 * x[:, :1]) * x[:, 1:2] + x[:, :1] ** 2, lambda x: np.cos(2 * x[:, 1:2]) + 0.5 * x[:, :1]]
    model = B.multi_outputGP(m, kernel=[B.kern.RBF(d, variance=1.0, lengthscale=0.3, ARD=True) for _ in range(m)], noise_var=[1e-4] * m, fixed_hyps=True)
    X0 = np.random.uniform(size=(12, 2))
    Y0 = [fj(X0) for fj in f]
    model.updateModel(X0, Y0)
    la = K.LookAhead.fit(["rbf", "rbf"], X0, [y[:, 0] for y in Y0], [1.0, 1.0], [np.full(2, 0.3)] * 2, [1e-4, 1e-4])
    support, prob = np.array([[0.5, 0.2], [0.1, 0.9]]), np.array([0.5, 0.5])
    return space, f, model, X0, la, support, prob


def _separated(alpha, gate):
    """The reference's 16 best and whether each of the first 16 gaps exceeds four times the value gate there."""
    full = np.argsort(-alpha, kind="stable")
    top, g = alpha[full[:17]], gate[full[:17]]
    return full[:16], bool(np.all(top[:-1] - top[1:] > 4 * np.maximum(g[:-1], g[1:])))


def test_classes_against_the_restatement_and_select_anchors():
    """The first 16 values of every case are separated by more than four times the value gate on the restatement alone (checked on the
    oracle's posterior with these seeds), so select_anchors(16) is compared in full for every class."""
    space, f, model, X0, la, support, prob = _surface_problem()
    U = B.Utility(parameter_dist=B.ParameterDistribution(support=support, prob_dist=prob), device="neg_sq_dist")
    Q = np.random.RandomState(3).uniform(size=(200, 2))
    post, postg = CR.posterior(la, Q), CR.posterior(la, Q[:NGRAD], grad=True)
    cases = ((B.uUCB, {"level": 0.9}, RR.QUANTILE), (B.uCVaR, {"level": 0.1}, RR.LOWER_TAIL), (B.uCVaR, {"level": 0.6, "tail": "upper"}, RR.UPPER_TAIL))
    for i, (cls, kw, kind) in enumerate(cases):
        acq = cls(model, space, utility=U, **kw)
        acq.W_samples = np.random.RandomState(50 + i).normal(size=(25, 2))
        k = RR.rank_of(kw["level"], 25)
        assert acq.rank == k
        ref = RR.risk(post[0], post[1], acq.W_samples, support, prob, "neg_sq_dist", None, kind, k)
        gate = 1e-5 * np.abs(ref["alpha"]) + 1e-12 * ref["scale"]
        got = acq._compute_acq(Q)
        assert got.shape == (200, 1)
        assert np.all(np.abs(got[:, 0] - ref["alpha"]) <= gate)
        best16, separated = _separated(ref["alpha"], gate)
        assert separated
        np.testing.assert_array_equal(acq.select_anchors(16), best16)
        refg = RR.risk(postg[0], postg[1], acq.W_samples, support, prob, "neg_sq_dist", None, kind, k, postg[2], postg[3])
        v, dv = acq._compute_acq_withGradients(Q[:NGRAD])
        keep = compared_rows(refg)
        assert v.shape == (NGRAD, 1) and dv.shape == (NGRAD, 2) and np.mean(~keep) <= 0.05
        assert np.all(np.abs(v[:, 0] - refg["alpha"]) <= 1e-5 * np.abs(refg["alpha"]) + 1e-12 * refg["scale"])
        np.testing.assert_allclose(dv[keep], refg["dalpha"][keep], rtol=1e-4, atol=1e-9 * max(1.0, np.abs(refg["dalpha"]).max()))
    lin = B.Utility(parameter_dist=B.ParameterDistribution(support=support, prob_dist=prob), linear=True)
    acq = B.maUCB(model, space, utility=lin, exploration_weight=1.5)
    want, g = RR.linear_ucb(postg[0], postg[1], support, prob, 1.5, postg[2], postg[3])
    ref = RR.linear_ucb(post[0], post[1], support, prob, 1.5)
    np.testing.assert_allclose(acq._compute_acq(Q)[:, 0], ref, rtol=1e-5, atol=1e-12)
    best16, separated = _separated(ref, 1e-5 * np.abs(ref) + 1e-12)
    assert separated
    np.testing.assert_array_equal(acq.select_anchors(16), best16)
    v, dv = acq._compute_acq_withGradients(Q[:NGRAD])
    np.testing.assert_allclose(v[:, 0], want, rtol=1e-5, atol=1e-12)
    np.testing.assert_allclose(dv, g, rtol=1e-4, atol=1e-9 * max(1.0, np.abs(g).max()))


def test_uucb_through_the_acquisition_optimizer_and_one_cbo_iteration():
    space, f, model, X0, la, support, prob = _surface_problem()
    U = B.Utility(parameter_dist=B.ParameterDistribution(support=support, prob_dist=prob), device="neg_sq_dist")
    opt = B.AcquisitionOptimizer(space, optimizer='lbfgs', n_starting=200, n_anchor=16)
    acq = B.uUCB(model, space, optimizer=opt, utility=U, level=0.9)
    x, fx = acq.optimize()
    assert x.shape == (1, 2) and np.all(x >= 0.0) and np.all(x <= 1.0)
    value = acq._compute_acq(x)[0, 0]
    anchors = opt.last_info["anchor_points"]
    assert len(anchors) == 16
    at_anchors = acq._compute_acq(anchors)[:, 0]
    print("uUCB optimum %.6g against its 16 anchors' best %.6g" % (value, at_anchors.max()))
    assert value == -float(np.squeeze(fx))
    assert value >= at_anchors.max()
    with pytest.raises(NotImplementedError, match="refine='device' does not cover uUCB"):
        B.uUCB(model, space, optimizer=B.AcquisitionOptimizer(space, optimizer='lbfgs', n_starting=50, n_anchor=4, refine="device"), utility=U).optimize()
    objective = B.MultiObjective(f, noise_var=[1e-4, 1e-4])
    bo = B.CBO(model, space, objective, acq, B.Sequential(acq), X0)
    bo.run_optimization(max_iter=1)
    assert bo.X.shape == (13, 2) and np.all(bo.X >= 0.0) and np.all(bo.X <= 1.0)


def test_every_refusal_names_its_entry_point_and_the_caches_are_left_alone():
    d, N = 2, 50
    kinds = MIXED[:3]
    X, Y, var, ls, nz, Xc = K.problem(kinds, N, d, 20, 9, noise=1e-4)
    lib, dp = _ffi.load(), _ffi.dptr
    th, out = np.zeros((2, 3)), np.empty(20)

    def bad(rc, name, text):
        msg = lib.bocf_last_error()
        assert rc < 0 and name.encode() in msg and text.encode() in msg, (rc, msg, text)
    fresh = _ffi.Context(0)
    bad(lib.bocf_acq_risk(fresh.handle, 0, 0, 1, None, 0, dp(th), 3, None, 2, dp(out), None), "bocf_acq_risk", "model not fitted")
    bad(lib.bocf_acq_linear_ucb(fresh.handle, 2.0, dp(th), None, 2, dp(out), None), "bocf_acq_linear_ucb", "model not fitted")
    fresh.close()
    model = _fixed_model(kinds, X, Y, var, ls, nz)
    model._ensure_fitted()
    h = model._context().handle

    def risk(kind=0, rank=0, util=_ffi.UTIL_NEG_SQ_DIST, theta=th, tdim=3, L=2, g=None):
        return lib.bocf_acq_risk(h, kind, rank, util, None, 0, dp(theta), tdim, None, L, dp(out), dp(g))
    assert lib.bocf_set_candidates(h, dp(_ffi.f64(Xc)), 20) == 0
    who = "bocf_acq_risk"
    bad(risk(), who, "no Monte-Carlo samples")
    model.set_mc_samples(np.random.RandomState(2).normal(size=(4, 3)))
    bad(risk(kind=3), who, "unknown risk kind")
    bad(risk(rank=-1), who, "rank out of range")
    bad(risk(rank=4), who, "rank out of range")
    bad(risk(util=_ffi.UTIL_PROGRAM), who, "BOCF_UTIL_PROGRAM")
    bad(risk(util=7), who, "unknown utility kind")
    bad(risk(L=0), who, "L out of range")
    bad(risk(theta=None), who, "theta")
    bad(risk(tdim=2), who, "theta_dim must equal m")
    bad(risk(util=_ffi.UTIL_ROSENBROCK, tdim=1), who, "even m")
    assert lib.bocf_set_candidates(h, dp(_ffi.f64(Xc)), 0) == 0
    bad(risk(), who, "no resident candidates")
    bad(lib.bocf_acq_linear_ucb(h, 2.0, dp(th), None, 2, dp(out), None), "bocf_acq_linear_ucb", "no resident candidates")
    assert lib.bocf_set_candidates(h, dp(_ffi.f64(Xc)), 20) == 0
    bad(lib.bocf_acq_linear_ucb(h, np.inf, dp(th), None, 2, dp(out), None), "bocf_acq_linear_ucb", "kappa must be finite")
    bad(lib.bocf_acq_linear_ucb(h, 2.0, None, None, 2, dp(out), None), "bocf_acq_linear_ucb", "theta")
    bad(lib.bocf_acq_linear_ucb(h, 2.0, dp(th), None, 33, dp(out), None), "bocf_acq_linear_ucb", "L out of range")
    # (the one refusal left, d > 64 with gradients, has no fitted context to happen on: a fit takes d <= 32 -- shown here for d = 65 -- so
    # tests/test_risk_cpu.py drives that branch of both entry points through the stand-alone driver of csrc/risk_args.h)
    X65, Y65, v65, l65, n65, _ = K.problem(kinds, 20, 65, 4, 3, noise=1e-4)
    with pytest.raises(_ffi.BocfHipError, match="N, d or m out of range"):
        _fixed_model(kinds, X65, Y65, v65, l65, n65)._ensure_fitted()
    assert risk(rank=3) == 0 and risk(rank=3, g=np.empty((20, d))) == 0
    assert lib.bocf_acq_linear_ucb(h, 2.0, dp(th), None, 2, dp(out), dp(np.empty((20, d)))) == 0
    # more samples than the selection holds
    model.set_mc_samples(np.random.RandomState(3).normal(size=(4097, 3)))
    bad(risk(), who, "S <= 4096")
    # the improvement acquisitions' parameters and best-so-far are left as they were: the same bits before and after
    rng = np.random.RandomState(0)
    support, prob, W = rng.uniform(-0.5, 0.5, size=(2, 3)), np.array([0.4, 0.6]), rng.normal(size=(25, 3))
    before = model.acq_mc(Xc, _ffi.ACQ_EI, _ffi.UTIL_NEG_SQ_DIST, None, support, prob, W=W)
    model.acq_risk(Xc, RR.LOWER_TAIL, 3, _ffi.UTIL_NEG_SQ_DIST, None, rng.uniform(size=(3, 3)), None, W=W, grad=True)
    model.acq_linear_ucb(Xc, 1.0, rng.uniform(size=(1, 3)), None, grad=True)
    np.testing.assert_array_equal(model.acq_mc(Xc, _ffi.ACQ_EI, _ffi.UTIL_NEG_SQ_DIST, None, support, prob, W=W), before)
    with pytest.raises(ValueError, match="output_dim"):
        model.acq_linear_ucb(Xc, 1.0, np.zeros((1, 2)), None)
