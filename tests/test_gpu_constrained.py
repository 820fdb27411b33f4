"""Constrained uEI on the device (bocf_set_output_constraints, bocf_feasible_best, bocf_acq_mc_constrained, multi_outputGP.set_output_constraints
/ feasible_best / acq_mc_constrained, uEI_constrained) against the NumPy restatement tests/constrained_ref.py -- never against another
device path alone.

Gates.  Kernel alone on a host-given posterior (bocf_set_posterior): rtol 1e-11, atol 1e-14, the project's canned Monte-Carlo gate, at
eta = 0.05 and at the default eta = 1e-3.  Through the model against the restatement on the oracle's posterior: values rtol 1e-5, atol 1e-12;
gradients (at most 40 candidates) rtol 1e-4, atol 1e-9 max(1, |g|max) -- the gates of acq_mc; eta = 0.05 and noise 1e-4 there, so that the
posterior's own error times 1 / eta stays inside them.  No value is excluded."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import constrained_ref as CR  # noqa: E402
import kg_ref as K  # noqa: E402

import bocf_amd as B  # noqa: E402
from bocf_amd import _ffi  # noqa: E402
from oracle import cpu_ref as R  # noqa: E402

pytestmark = pytest.mark.gpu

KERN = {"rbf": B.kern.RBF, "se": B.kern.SE, "matern52": B.kern.Matern52, "matern32": B.kern.Matern32}
KID = {"rbf": _ffi.KERN_RBF, "se": _ffi.KERN_SE, "matern52": _ffi.KERN_MATERN52, "matern32": _ffi.KERN_MATERN32}
UTIL = {"linear": _ffi.UTIL_LINEAR, "neg_sq_dist": _ffi.UTIL_NEG_SQ_DIST, "neg_sum_exp": _ffi.UTIL_NEG_SUM_EXP,
        "neg_exp_cos": _ffi.UTIL_NEG_EXP_COS, "rosenbrock": _ffi.UTIL_ROSENBROCK}
MIXED = ["se", "matern52", "rbf", "matern32"]           # one family per output
NGRAD = 40

#        N    d  m  K  S   L  C    H  utility        prob
BASE = (120, 3, 4, 2, 25, 3, 129, 1, "neg_sq_dist", True)


def _vary(**kw):
    names = ("N", "d", "m", "K", "S", "L", "C", "H", "kind", "prob")
    c = dict(zip(names, BASE))
    c.update(kw)
    return tuple(c[n] for n in names)


CASES = ([BASE]
         + [_vary(C=C, N=64) for C in (1, 3, 4, 5, 257)]                                   # workgroup tail
         + [_vary(S=S, N=100) for S in (1, 63, 64, 65, 130)]                               # lane stride
         + [_vary(K=1), _vary(K=8)]
         + [_vary(m=1, N=64), _vary(m=2, N=64, kind="rosenbrock"), _vary(m=8, N=64), _vary(m=9, N=64), _vary(m=16, N=64, kind="rosenbrock")]
         + [_vary(L=1, prob=False), _vary(L=1), _vary(L=3, prob=False)]
         + [_vary(d=1, N=64), _vary(d=6, N=200)]
         + [_vary(H=2, N=100)]                                                             # best_group = the second hyper-sample
         + [_vary(kind=k, N=100) for k in ("linear", "neg_sum_exp", "neg_exp_cos", "rosenbrock")])
IDS = ["N%d-d%d-m%d-K%d-S%d-L%d-C%d-H%d-%s-%s" % (c[:9] + ("prob" if c[9] else "mean",)) for c in CASES]


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
    N, d, m, Kc, S, L, C, H, kind, with_prob = case
    seed = 1000 + CASES.index(case) if case in CASES else 999
    kinds = [MIXED[j % 4] for j in range(m)]
    X, Y, var, ls, nz, Xc = K.problem(kinds, N, d, C, seed, noise=1e-4)
    las = [K.LookAhead.fit(kinds, X, Y, var * (1 + 0.1 * h), ls * (1 - 0.05 * h), nz) for h in range(H)]
    rng = np.random.RandomState(7000 + seed)
    W = rng.normal(size=(S, m))
    thetas, params = CR.utility_inputs(rng, kind, m, L)
    prob = rng.dirichlet(np.ones(L)) if with_prob else None
    mts = [CR.train_mean(la) for la in las]
    A, b, eta = CR.draw_constraints(rng, mts[H - 1], Kc, 0.05, share=0.15)       # few feasible training points: a weak incumbent, many improving samples
    return dict(kinds=kinds, X=X, Y=Y, var=var, ls=ls, nz=nz, Xc=Xc, las=las, W=W, thetas=thetas, params=params, prob=prob, mts=mts,
                A=A, b=b, eta=eta, kind=kind, H=H)


_CACHE = {}


def _case(case):
    """(inputs, device model, restatement of all candidates, restatement with gradients of the first NGRAD), made once per case."""
    if case not in _CACHE:
        inp = _inputs(case)
        a = (inp["kinds"], inp["X"], inp["Y"], inp["var"], inp["ls"], inp["nz"])
        model = _fixed_model(*a) if inp["H"] == 1 else _hyper_model(*a, inp["H"])
        H = inp["H"]
        post = [CR.posterior(la, inp["Xc"]) for la in inp["las"]]
        u = (inp["W"], inp["thetas"], inp["prob"], inp["kind"], inp["params"], inp["A"], inp["b"], inp["eta"])
        ref = CR.constrained_hyper([p[0] for p in post], [p[1] for p in post], inp["mts"], *u, best_group=H - 1)
        pg = [CR.posterior(la, inp["Xc"][:NGRAD], grad=True) for la in inp["las"]]
        refg = CR.constrained_hyper([p[0] for p in pg], [p[1] for p in pg], inp["mts"], *u, dmeans=[p[2] for p in pg], dvars=[p[3] for p in pg],
                                    best_group=H - 1)
        _CACHE.clear()                                    # one case's model and references at a time
        _CACHE[case] = (inp, model, ref, refg)
    return _CACHE[case]


def _device(model, inp, X, grad=False, oc=None):
    model.set_hyperparameters(inp["H"] - 1)   # the incumbent is that of the hyper-sample current on entry: the last one here
    model.set_output_constraints(oc or B.OutputConstraints(inp["A"], inp["b"], inp["eta"]))
    return model.acq_mc_constrained(X, UTIL[inp["kind"]], inp["params"], inp["thetas"], inp["prob"], W=inp["W"], grad=grad)


# ---- the kernels alone, on a host-given posterior --------------------------------------------------------------------------------------
@pytest.mark.parametrize("eta", [0.05, 1e-3])
@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_kernel_on_a_canned_posterior(case, eta):
    N, d, m, Kc, S, L, C, H, kind, with_prob = case
    rng = np.random.RandomState(300 + CASES.index(case))
    mean, var = rng.uniform(-1.0, 1.0, size=(H * m, C)), rng.uniform(0.01, 0.5, size=(H * m, C))
    mt = rng.uniform(-1.0, 1.0, size=(H * m, N))
    W = rng.normal(size=(S, m))
    thetas, params = CR.utility_inputs(rng, kind, m, L)
    prob = rng.dirichlet(np.ones(L)) if with_prob else None
    A, b, _ = CR.draw_constraints(rng, mt[(H - 1) * m:], Kc, eta)
    etas = np.full(Kc, eta)
    sl = [slice(h * m, (h + 1) * m) for h in range(H)]
    ref = CR.constrained_hyper([mean[s] for s in sl], [var[s] for s in sl], [mt[s] for s in sl], W, thetas, prob, kind, params, A, b, etas,
                               best_group=H - 1)
    lib, ctx, dp = _ffi.load(), _ffi.Context(0), _ffi.dptr
    h = ctx.handle
    _ffi.check(lib.bocf_set_posterior(h, H * m, C, N, dp(_ffi.f64(mean)), dp(_ffi.f64(var)), dp(_ffi.f64(mt))), "bocf_set_posterior")
    ctx.set_option("hyper_samples", H)
    ctx.set_option("best_group", H - 1)
    _ffi.check(lib.bocf_set_mc_samples(h, dp(_ffi.f64(W)), S), "bocf_set_mc_samples")
    _ffi.check(lib.bocf_set_output_constraints(h, dp(_ffi.f64(A)), dp(_ffi.f64(b)), dp(etas), Kc, m), "bocf_set_output_constraints")
    th, par, pr = _ffi.f64(thetas), None if params is None else _ffi.f64(params), None if prob is None else _ffi.f64(prob)
    util = (UTIL[kind], dp(par), 0 if par is None else par.size, dp(th), th.shape[1])
    got = np.empty(C)
    _ffi.check(lib.bocf_acq_mc_constrained(h, *util, dp(pr), L, dp(got), None), "bocf_acq_mc_constrained")
    best, nf = np.empty(L), _ffi.ctypes.c_longlong()
    _ffi.check(lib.bocf_feasible_best(h, *util, L, dp(best), _ffi.ctypes.byref(nf)), "bocf_feasible_best")
    err = np.abs(got - ref["alpha"])
    print("canned %s eta %g: max alpha %.3g, share > 0 %.2f, |F| %d, max abs err %.3g, max rel err %.3g"
          % (IDS[CASES.index(case)], eta, ref["alpha"].max(), np.mean(ref["alpha"] > 0), nf.value, err.max(),
             np.max(err / np.maximum(np.abs(ref["alpha"]), 1e-300) * (ref["alpha"] > 0))))
    assert nf.value == ref["n_feasible"]
    np.testing.assert_allclose(best, ref["best"], rtol=1e-13)
    assert np.all(np.isfinite(got)) and np.all(got >= 0)
    np.testing.assert_allclose(got, ref["alpha"], rtol=1e-11, atol=1e-14)
    # the gradient form is refused by name on a host-given posterior
    assert lib.bocf_acq_mc_constrained(h, *util, dp(pr), L, dp(got), dp(np.empty((C, 1)))) < 0
    msg = lib.bocf_last_error()
    assert b"bocf_acq_mc_constrained" in msg and b"host-given posterior" in msg
    ctx.close()


def test_selection_after_the_call_is_the_restatements_stable_argsort():
    """No feasible training point: alpha is the smoothed probability of feasibility, positive and distinct for every candidate."""
    rng = np.random.RandomState(17)
    m, C, N, S = 4, 129, 64, 25
    mean, var, mt = rng.uniform(-1, 1, size=(m, C)), rng.uniform(0.01, 0.5, size=(m, C)), rng.uniform(-1, 1, size=(m, N))
    W, thetas = rng.normal(size=(S, m)), rng.uniform(-0.5, 0.5, size=(3, m))
    A, b, eta = np.array([[1.0, 0.5, 0.0, 0.0], [0.0, 0.0, -1.0, 0.3]]), np.array([-1.6, -1.4]), np.full(2, 0.05)
    ref = CR.constrained(mean, var, mt, W, thetas, None, "neg_sq_dist", None, A, b, eta)
    assert ref["n_feasible"] == 0
    order = np.argsort(-ref["alpha"], kind="stable")[:16]
    top = ref["alpha"][np.argsort(-ref["alpha"], kind="stable")[:17]]
    assert np.all(top[:-1] - top[1:] > 1e-9 * top[:-1])            # the first 16 are separated by far more than the kernel's error
    lib, ctx, dp = _ffi.load(), _ffi.Context(0), _ffi.dptr
    h = ctx.handle
    _ffi.check(lib.bocf_set_posterior(h, m, C, N, dp(_ffi.f64(mean)), dp(_ffi.f64(var)), dp(_ffi.f64(mt))), "bocf_set_posterior")
    _ffi.check(lib.bocf_set_mc_samples(h, dp(_ffi.f64(W)), S), "bocf_set_mc_samples")
    _ffi.check(lib.bocf_set_output_constraints(h, dp(A), dp(b), dp(eta), 2, m), "bocf_set_output_constraints")
    _ffi.check(lib.bocf_acq_mc_constrained(h, _ffi.UTIL_NEG_SQ_DIST, None, 0, dp(_ffi.f64(thetas)), m, None, 3, None, None), "bocf_acq_mc_constrained")
    idx, val = np.empty(16, dtype=np.int64), np.empty(16)
    _ffi.check(lib.bocf_select_topk(h, 16, idx.ctypes.data_as(_ffi._c_ll_p), dp(val)), "bocf_select_topk")
    np.testing.assert_array_equal(idx, order)
    np.testing.assert_allclose(val, ref["alpha"][order], rtol=1e-11, atol=1e-14)
    ctx.close()


# ---- through the model, against the restatement on the oracle's posterior ----------------------------------------------------------------
@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_values_against_the_restatement(case):
    inp, model, ref, _ = _case(case)
    got = _device(model, inp, inp["Xc"])
    best, nf = model.feasible_best(UTIL[inp["kind"]], inp["params"], inp["thetas"])
    err = np.abs(got - ref["alpha"])
    print("constrained %s: max alpha %.3g, share > 0 %.2f, |F| %d of %d, max abs err %.3g, max rel err %.3g"
          % (IDS[CASES.index(case)], ref["alpha"].max(), np.mean(ref["alpha"] > 0), nf, case[0], err.max(),
             np.max(err / np.maximum(np.abs(ref["alpha"]), 1e-300) * (ref["alpha"] > 0))))
    assert got.shape == (case[6],) and np.all(np.isfinite(got)) and np.all(got >= 0)
    assert nf == ref["n_feasible"]
    np.testing.assert_allclose(best, ref["best"], rtol=1e-6, atol=1e-9)
    np.testing.assert_allclose(got, ref["alpha"], rtol=1e-5, atol=1e-12)
    np.testing.assert_array_equal(_device(model, inp, inp["Xc"]), got)          # a second identical call: the same bits


@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_gradients_against_the_restatement(case):
    inp, model, _, ref = _case(case)
    X = inp["Xc"][:NGRAD]
    got, dgot = _device(model, inp, X, grad=True)
    assert dgot.shape == X.shape
    g = ref["dalpha"]
    print("constrained gradient %s: %d candidates, %d with a nonzero gradient, max abs err %.3g, gradient scale %.3g"
          % (IDS[CASES.index(case)], len(X), np.sum(np.any(g != 0, 1)), np.abs(dgot - g).max(), np.abs(g).max()))
    np.testing.assert_allclose(got, ref["alpha"], rtol=1e-5, atol=1e-12)
    np.testing.assert_allclose(dgot, g, rtol=1e-4, atol=1e-9 * max(1.0, np.abs(g).max()))


def test_vacuous_constraints_give_acq_mc():
    inp, model, _, _ = _case(BASE)
    oc = B.OutputConstraints(inp["A"], np.full(len(inp["b"]), 1e30), inp["eta"])
    got = _device(model, inp, inp["Xc"], oc=oc)
    want = model.acq_mc(inp["Xc"], _ffi.ACQ_EI, UTIL[inp["kind"]], inp["params"], inp["thetas"], inp["prob"], W=inp["W"])
    assert want.max() > 0
    np.testing.assert_allclose(got, want, rtol=1e-12, atol=0)
    assert model.feasible_best(UTIL[inp["kind"]], inp["params"], inp["thetas"])[1] == BASE[0]


def test_no_feasible_training_point_and_exactly_one():
    inp, model, _, _ = _case(BASE)
    mt, kind = inp["mts"][0], inp["kind"]
    post = CR.posterior(inp["las"][0], inp["Xc"])
    order = np.argsort(mt[0])
    e0 = np.zeros((1, BASE[2]))
    e0[0, 0] = 1.0
    # y_0 <= a level below every training mean: F is empty, alpha is the smoothed probability of feasibility
    oc = B.OutputConstraints(e0, [mt[0, order[0]] - 0.3], eta=0.05)
    got = _device(model, inp, inp["Xc"], oc=oc)
    best, nf = model.feasible_best(UTIL[kind], inp["params"], inp["thetas"])
    assert nf == 0 and np.all(best == -np.inf)
    ref = CR.constrained(post[0], post[1], mt, inp["W"], inp["thetas"], inp["prob"], kind, inp["params"], oc.A, oc.b, oc.eta)
    assert ref["n_feasible"] == 0 and ref["alpha"].max() > 1e-3
    np.testing.assert_allclose(ref["alpha"], ref["phi_mean"] * np.sum(inp["prob"]), rtol=1e-13)
    np.testing.assert_allclose(got, ref["alpha"], rtol=1e-5, atol=1e-12)
    pg = CR.posterior(inp["las"][0], inp["Xc"][:NGRAD], grad=True)
    refg = CR.constrained(pg[0], pg[1], mt, inp["W"], inp["thetas"], inp["prob"], kind, inp["params"], oc.A, oc.b, oc.eta, pg[2], pg[3])["dalpha"]
    dgot = _device(model, inp, inp["Xc"][:NGRAD], grad=True, oc=oc)[1]
    assert np.abs(refg).max() > 1e-4                               # (a gradient to compare: the restatement's, 8.4e-4 here)
    np.testing.assert_allclose(dgot, refg, rtol=1e-4, atol=1e-9 * max(1.0, np.abs(refg).max()))
    # ... between the lowest and the second lowest: that one point is the incumbent
    oc = B.OutputConstraints(e0, [0.5 * (mt[0, order[0]] + mt[0, order[1]])], eta=0.05)
    got = _device(model, inp, inp["Xc"], oc=oc)
    best, nf = model.feasible_best(UTIL[kind], inp["params"], inp["thetas"])
    assert nf == 1
    mu_dev = model.posterior_mean_at_evaluated_points()
    np.testing.assert_allclose(best, [R.utility_eval(kind, th, mu_dev[:, order[0]], inp["params"]) for th in inp["thetas"]], rtol=1e-12)
    ref = CR.constrained(post[0], post[1], mt, inp["W"], inp["thetas"], inp["prob"], kind, inp["params"], oc.A, oc.b, oc.eta)
    assert ref["n_feasible"] == 1
    np.testing.assert_allclose(got, ref["alpha"], rtol=1e-5, atol=1e-12)


def test_batch_independence_bit_for_bit():
    case = _vary(C=257, N=64)
    inp, model, _, _ = _case(case)
    Xc = inp["Xc"]
    whole = _device(model, inp, Xc)
    for cut in (128, 101):
        np.testing.assert_array_equal(np.concatenate([_device(model, inp, Xc[:cut]), _device(model, inp, Xc[cut:])]), whole)
    # the predict pass's chunking: the same bits in chunks of 128 candidates
    model.set_option("chunk", 128)
    np.testing.assert_array_equal(_device(model, inp, Xc), whole)
    model.set_option("chunk", 65536)


def test_state_is_left_alone_and_the_constraints_survive_model_changes():
    d, N, C = 3, 100, 60
    kinds = MIXED[:3]
    X, Y, var, ls, nz, Xc = K.problem(kinds, N, d, C, 5, noise=1e-4)
    model = _fixed_model(kinds, X, Y, var, ls, nz)
    rng = np.random.RandomState(0)
    support, prob = rng.uniform(-0.5, 0.5, size=(2, 3)), np.array([0.4, 0.6])
    W = rng.normal(size=(25, 3))
    oc = B.OutputConstraints.bounds([None, -0.5, None], [0.4, None, None], eta=0.05)
    kind = _ffi.UTIL_NEG_SQ_DIST
    lib, h, dp = _ffi.load(), model._context().handle, _ffi.dptr
    A, Zf = rng.uniform(size=(9, d)), rng.normal(size=(4, 3))
    P, Zp = rng.uniform(size=(5, d)), rng.normal(size=(25, 3, 5))
    np.random.seed(3)
    model.set_reference_points(A)
    model.set_pending_points(P, Zp, W=W)
    model.draw_paths(3, 64)

    def others():
        return (model.acq_kg(Xc, "closed", kind, None, support, prob, Zf), model.acq_pending(Xc, kind, None, support, prob, W=W),
                model.path_values(Xc[:7]), model.acq_mc(Xc, _ffi.ACQ_EI, kind, None, support, prob, W=W))
    before = others()
    keys = (model._resident.reference, model._resident.pending, model._resident.paths)
    model.set_output_constraints(oc)
    a1 = model.acq_mc_constrained(Xc, kind, None, support, prob, W=W)
    model.acq_mc_constrained(Xc[:20], kind, None, support, prob, W=W, grad=True)
    assert (model._resident.reference, model._resident.pending) == keys[:2] and model._resident.paths is keys[2]
    for x, y in zip(before, others()):
        np.testing.assert_array_equal(x, y)
    np.testing.assert_array_equal(model.acq_mc_constrained(Xc, kind, None, support, prob, W=W), a1)
    # new targets (bocf_update_targets), an appended observation (bocf_append) and a refit (bocf_fit): the constraints stay resident --
    # the C call works without sending them again, and answers for the new posterior
    th, out = _ffi.f64(support), np.empty(C)
    for change in ("targets", "append", "refit"):
        if change == "targets":
            Y = [y + 0.05 for y in Y]
        elif change == "append":
            X, Y = np.concatenate([X, Xc[:1]]), [np.concatenate([y, [0.2]]) for y in Y]
        else:
            model.incremental = False
        model.updateModel(X, [y[:, None] for y in Y])
        model._ensure_fitted()
        assert model._resident.constraints == oc.key()
        model.set_mc_samples(W)
        assert lib.bocf_set_candidates(h, dp(_ffi.f64(Xc)), C) == 0
        assert lib.bocf_acq_mc_constrained(h, kind, None, 0, dp(th), 3, dp(_ffi.f64(prob)), 2, dp(out), None) == 0, (change, lib.bocf_last_error())
        la = K.LookAhead.fit(kinds, X, Y, var, ls, nz)
        post = CR.posterior(la, Xc)
        ref = CR.constrained(post[0], post[1], CR.train_mean(la), W, support, prob, "neg_sq_dist", None, oc.A, oc.b, oc.eta)
        np.testing.assert_allclose(out, ref["alpha"], rtol=1e-5, atol=1e-12)
    # dropped on request; the next call says so
    model.set_output_constraints(None)
    assert lib.bocf_acq_mc_constrained(h, kind, None, 0, dp(th), 3, None, 2, dp(out), None) < 0
    assert b"bocf_acq_mc_constrained" in lib.bocf_last_error() and b"no output constraints" in lib.bocf_last_error()
    with pytest.raises(RuntimeError, match="constraints"):
        model.acq_mc_constrained(Xc, kind, None, support, prob, W=W)


def test_every_refusal_names_its_entry_point():
    d, N = 2, 50
    kinds = MIXED[:3]
    X, Y, var, ls, nz, Xc = K.problem(kinds, N, d, 20, 9, noise=1e-4)
    lib, dp = _ffi.load(), _ffi.dptr
    A, b, eta, th, out = np.ones((2, 3)), np.zeros(2), np.full(2, 0.1), np.zeros((2, 3)), np.empty(20)

    def bad(rc, name, text):
        msg = lib.bocf_last_error()
        assert rc < 0 and name.encode() in msg and text.encode() in msg, (rc, msg, text)
    fresh = _ffi.Context(0)
    assert lib.bocf_set_output_constraints(fresh.handle, dp(A), dp(b), dp(eta), 2, 3) == 0      # no fit needed to stage them
    bad(lib.bocf_acq_mc_constrained(fresh.handle, 1, None, 0, dp(th), 3, None, 2, dp(out), None), "bocf_acq_mc_constrained", "model not fitted")
    bad(lib.bocf_feasible_best(fresh.handle, 1, None, 0, dp(th), 3, 2, dp(out), None), "bocf_feasible_best", "model not fitted")
    fresh.close()
    model = _fixed_model(kinds, X, Y, var, ls, nz)
    model._ensure_fitted()
    h = model._context().handle

    def acq(util=_ffi.UTIL_NEG_SQ_DIST, theta=th, tdim=3, L=2, g=None):
        return lib.bocf_acq_mc_constrained(h, util, None, 0, dp(theta), tdim, None, L, dp(out), dp(g))
    assert lib.bocf_set_candidates(h, dp(_ffi.f64(Xc)), 20) == 0
    who = "bocf_acq_mc_constrained"
    bad(acq(), who, "no output constraints")
    bad(lib.bocf_feasible_best(h, 1, None, 0, dp(th), 3, 2, dp(out), None), "bocf_feasible_best", "no output constraints")
    bad(lib.bocf_set_output_constraints(h, dp(A), dp(b), dp(eta), 2, 2), "bocf_set_output_constraints", "m differs")
    bad(lib.bocf_set_output_constraints(h, dp(A), dp(b), dp(eta), 9, 3), "bocf_set_output_constraints", "K out of range")
    bad(lib.bocf_set_output_constraints(h, dp(A), dp(np.array([0.0, np.inf])), dp(eta), 2, 3), "bocf_set_output_constraints", "non-finite")
    bad(lib.bocf_set_output_constraints(h, dp(A), dp(b), dp(np.array([0.1, 0.0])), 2, 3), "bocf_set_output_constraints", "eta must be")
    assert lib.bocf_set_output_constraints(h, dp(A), dp(b), dp(eta), 2, 3) == 0
    bad(acq(), who, "no Monte-Carlo samples")
    model.set_mc_samples(np.random.RandomState(2).normal(size=(4, 3)))
    bad(acq(util=_ffi.UTIL_PROGRAM), who, "BOCF_UTIL_PROGRAM")
    bad(acq(util=7), who, "unknown utility kind")
    bad(acq(L=0), who, "L out of range")
    bad(acq(theta=None), who, "theta")
    bad(acq(tdim=2), who, "theta_dim must equal m")
    bad(acq(util=_ffi.UTIL_ROSENBROCK, tdim=1), who, "even m")
    assert lib.bocf_set_candidates(h, dp(_ffi.f64(Xc)), 0) == 0
    bad(acq(), who, "no resident candidates")
    assert lib.bocf_set_candidates(h, dp(_ffi.f64(Xc)), 20) == 0
    assert acq() == 0 and acq(g=np.empty((20, d))) == 0
    # the hyper-sample layout changed under resident constraints: m no longer matches
    model.set_option("hyper_samples", 3)
    bad(acq(), who, "another m")
    model.set_option("hyper_samples", 1)           # (a change of the layout forgets the device's Monte-Carlo samples)
    Wd = _ffi.f64(np.random.RandomState(2).normal(size=(4, 3)))
    assert lib.bocf_set_mc_samples(h, dp(Wd), 4) == 0 and acq() == 0


# ---- end to end ---------------------------------------------------------------------------------------------------------------------------
def test_uei_constrained_through_the_acquisition_optimizer():
    np.random.seed(41)
    d, m = 2, 2
    space = B.Design_space([{'name': 'x', 'type': 'continuous', 'domain': (0, 1), 'dimensionality': d}])
    f = [lambda x: np.sin(3 * x[:, :1]) * x[:, 1:2] + x[:, :1] ** 2, lambda x: np.cos(2 * x[:, 1:2]) + 0.5 * x[:, :1]]
    model = B.multi_outputGP(m, kernel=[B.kern.RBF(d, variance=1.0, lengthscale=0.3, ARD=True) for _ in range(m)], noise_var=[1e-4] * m, fixed_hyps=True)
    U = B.Utility(parameter_dist=B.ParameterDistribution(support=np.array([[0.5, 0.2], [0.1, 0.9]]), prob_dist=np.array([0.5, 0.5])), device="neg_sq_dist")
    opt = B.AcquisitionOptimizer(space, optimizer='lbfgs', n_starting=200, n_anchor=16)
    oc = B.OutputConstraints.bounds([None, 0.6], [0.9, None], eta=0.05)
    acq = B.uEI_constrained(model, space, optimizer=opt, utility=U, constraints=oc)
    X0 = np.random.uniform(size=(12, 2))
    Y0 = [fj(X0) for fj in f]
    model.updateModel(X0, Y0)
    x, fx = acq.optimize()
    assert x.shape == (1, 2) and np.all(x >= 0.0) and np.all(x <= 1.0)
    value = acq._compute_acq(x)[0, 0]
    anchors = opt.last_info["anchor_points"]
    assert len(anchors) == 16
    at_anchors = acq._compute_acq(anchors)[:, 0]
    print("uEI_constrained optimum %.6g against its 16 anchors' best %.6g" % (value, at_anchors.max()))
    assert value == -float(np.squeeze(fx)) and value > 0
    assert np.all(value >= at_anchors)
    # against the restatement at the optimum and the anchors
    la = K.LookAhead.fit(["rbf", "rbf"], X0, [y[:, 0] for y in Y0], [1.0, 1.0], [np.full(2, 0.3)] * 2, [1e-4, 1e-4])
    Q = np.concatenate([x, anchors])
    post = CR.posterior(la, Q)
    ref = CR.constrained(post[0], post[1], CR.train_mean(la), acq.W_samples, U.parameter_dist.support, acq.utility_prob_dist, "neg_sq_dist", None,
                         oc.A, oc.b, oc.eta)
    np.testing.assert_allclose(acq._compute_acq(Q)[:, 0], ref["alpha"], rtol=1e-5, atol=1e-12)
    # ... and as the acquisition of one CBO iteration
    objective = B.MultiObjective(f, noise_var=[1e-4, 1e-4])
    bo = B.CBO(model, space, objective, acq, B.Sequential(acq), X0)
    bo.run_optimization(max_iter=1)
    assert bo.X.shape == (13, 2) and np.all(bo.X >= 0.0) and np.all(bo.X <= 1.0)
