"""The feasibility-aware recommendation step on the device (bocf_train_utility_range, bocf_expected_utility_constrained,
multi_outputGP.train_utility_range / expected_utility_constrained, current_marginal_argmaxes and CBO with constraints) against the NumPy
restatement tests/ceu_ref.py -- never against another device path alone.

Gates (those of section 17, the gates on G scaled by n_h S because G is a sum where alpha was a mean; n_h = the
hyper-samples visited, scale = the largest |U - u0| the restatement met).  Kernel alone on a host-given posterior (bocf_set_posterior):
G rtol 1e-11, atol 1e-14 n_h S scale; P rtol 1e-11; at eta = 0.05 and at the default eta = 1e-3.  Through the model against the
restatement on the oracle's noiseless clipped posterior: G rtol 1e-5, atol 1e-12 n_h S scale; gradients (at most 40 candidates) rtol
1e-4, atol 1e-9 max(1, |g|max); eta = 0.05 and noise 1e-4 there.  No value is excluded.  Worst errors measured on an MI355X:
profiles/ceu/gpu_tests.txt."""
import ctypes
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import ceu_ref as CE  # noqa: E402
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
c_int_p = ctypes.POINTER(ctypes.c_int)

#        N    d  m  K  S   L  C    H  utility        u0 given
BASE = (120, 3, 4, 2, 25, 3, 129, 1, "neg_sq_dist", False)


def _vary(**kw):
    names = ("N", "d", "m", "K", "S", "L", "C", "H", "kind", "given")
    c = dict(zip(names, BASE))
    c.update(kw)
    return tuple(c[n] for n in names)


CASES = ([BASE, _vary(given=True)]
         + [_vary(C=C, N=64) for C in (1, 3, 4, 5, 257)]                                   # four waves per workgroup
         + [_vary(S=S, N=100) for S in (1, 63, 64, 65, 130)]                               # lane stride
         + [_vary(K=1), _vary(K=8, given=True)]
         + [_vary(m=1, N=64), _vary(m=2, N=64, kind="rosenbrock"), _vary(m=8, N=64, given=True), _vary(m=9, N=64), _vary(m=16, N=64, kind="rosenbrock")]
         + [_vary(L=1), _vary(L=1, given=True)]
         + [_vary(d=1, N=64), _vary(d=6, N=200)]
         + [_vary(H=2, N=100), _vary(H=2, N=100, given=True)]
         + [_vary(kind=k, N=100, given=g) for k, g in (("linear", True), ("neg_sum_exp", False), ("neg_exp_cos", True), ("rosenbrock", False))])
IDS = ["N%d-d%d-m%d-K%d-S%d-L%d-C%d-H%d-%s-%s" % (c[:9] + ("given" if c[9] else "default",)) for c in CASES]


def _n_hyps(H):
    return 3 if H == 1 else H                             # one resident hyper-sample: counted three times (the scale)


def _train_range(mt, thetas, kind, params):
    u = np.array([R.utility_eval(kind, th, mt, params) for th in np.atleast_2d(thetas)])
    return u.min(1), u.max(1)


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
    N, d, m, Kc, S, L, C, H, kind, given = case
    seed = 2000 + CASES.index(case) if case in CASES else 1999
    kinds = [MIXED[j % 4] for j in range(m)]
    X, Y, var, ls, nz, Xc = K.problem(kinds, N, d, C, seed, noise=1e-4)
    las = [K.LookAhead.fit(kinds, X, Y, var * (1 + 0.1 * h), ls * (1 - 0.05 * h), nz) for h in range(H)]
    rng = np.random.RandomState(8000 + seed)
    Z = rng.normal(size=(L, S, m))
    thetas, params = CR.utility_inputs(rng, kind, m, L)
    mts = [CR.train_mean(la) for la in las]
    A, b, eta = CR.draw_constraints(rng, mts[0], Kc, 0.05, share=0.5)
    # the default is the train minimum of the hyper-sample current on entry (the first here); the given one lies below every utility met
    u0 = _train_range(mts[0], thetas, kind, params)[0] - (rng.uniform(0.5, 1.5, size=L) if given else 0.0)
    return dict(kinds=kinds, X=X, Y=Y, var=var, ls=ls, nz=nz, Xc=Xc, las=las, Z=Z, thetas=thetas, params=params, mts=mts, A=A, b=b, eta=eta,
                kind=kind, H=H, rows=np.arange(C) % L, u0=u0, given=given)


_CACHE = {}


def _case(case):
    """(inputs, device model, restatement of all candidates, restatement with gradients of the first NGRAD), made once per case."""
    if case not in _CACHE:
        inp = _inputs(case)
        a = (inp["kinds"], inp["X"], inp["Y"], inp["var"], inp["ls"], inp["nz"])
        model = _fixed_model(*a) if inp["H"] == 1 else _hyper_model(*a, inp["H"])
        nh = _n_hyps(inp["H"])
        u = (inp["kind"], inp["params"], inp["A"], inp["b"], inp["eta"], nh)
        post = [CE.posterior_noiseless(la, inp["Xc"]) for la in inp["las"]]
        ref = CE.constrained_eu_hyper([p[0] for p in post], [p[1] for p in post], inp["Z"], inp["thetas"], inp["rows"], inp["u0"], *u)
        pg = [CE.posterior_noiseless(la, inp["Xc"][:NGRAD], grad=True) for la in inp["las"]]
        refg = CE.constrained_eu_hyper([p[0] for p in pg], [p[1] for p in pg], inp["Z"], inp["thetas"], inp["rows"][:NGRAD], inp["u0"], *u,
                                       dmeans=[p[2] for p in pg], dvars=[p[3] for p in pg])
        _CACHE.clear()                                    # one case's model and references at a time
        _CACHE[case] = (inp, model, ref, refg)
    return _CACHE[case]


def _device(model, inp, X, rows, grad=False, oc=None, u0=None):
    """The public path; the default u0 is the device's own train_utility_range minimum, as the recommendation step takes it."""
    model.set_hyperparameters(0)
    model.set_output_constraints(oc or B.OutputConstraints(inp["A"], inp["b"], inp["eta"]))
    if u0 is None:
        u0 = inp["u0"] if inp["given"] else model.train_utility_range(UTIL[inp["kind"]], inp["params"], inp["thetas"])[0]
    return model.expected_utility_constrained(X, UTIL[inp["kind"]], inp["thetas"], rows, u0, inp["Z"], n_hyps=_n_hyps(inp["H"]), grad=grad,
                                              util_params=inp["params"])


# ---- the kernels alone, on a host-given posterior --------------------------------------------------------------------------------------
@pytest.mark.parametrize("eta", [0.05, 1e-3])
@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_kernel_on_a_canned_posterior(case, eta):
    N, d, m, Kc, S, L, C, H, kind, given = case
    rng = np.random.RandomState(400 + CASES.index(case))
    mean, var = rng.uniform(-1.0, 1.0, size=(H * m, C)), rng.uniform(0.01, 0.5, size=(H * m, C))
    mt = rng.uniform(-1.0, 1.0, size=(H * m, N))
    Z = rng.normal(size=(L, S, m))
    thetas, params = CR.utility_inputs(rng, kind, m, L)
    A, b, _ = CR.draw_constraints(rng, mt[:m], Kc, eta)
    etas = np.full(Kc, eta)
    rows = (np.arange(C) % L).astype(np.int32)
    lo, hi = _train_range(mt[:m], thetas, kind, params)
    u0 = lo - rng.uniform(0.5, 1.5, size=L) if given else lo
    sl = [slice(h * m, (h + 1) * m) for h in range(H)]
    nh = _n_hyps(H)
    ref = CE.constrained_eu_hyper([mean[s] for s in sl], [var[s] for s in sl], Z, thetas, rows, u0, kind, params, A, b, etas, nh)
    lib, ctx, dp = _ffi.load(), _ffi.Context(0), _ffi.dptr
    h = ctx.handle
    _ffi.check(lib.bocf_set_posterior(h, H * m, C, N, dp(_ffi.f64(mean)), dp(_ffi.f64(var)), dp(_ffi.f64(mt))), "bocf_set_posterior")
    ctx.set_option("hyper_samples", H)
    _ffi.check(lib.bocf_set_eu_samples(h, dp(_ffi.f64(Z)), L, S), "bocf_set_eu_samples")
    _ffi.check(lib.bocf_set_output_constraints(h, dp(_ffi.f64(A)), dp(_ffi.f64(b)), dp(etas), Kc, m), "bocf_set_output_constraints")
    th, par = _ffi.f64(thetas), None if params is None else _ffi.f64(params)
    util = (UTIL[kind], dp(par), 0 if par is None else par.size, dp(th), th.shape[1], L)
    dlo, dhi = np.empty(L), np.empty(L)
    _ffi.check(lib.bocf_train_utility_range(h, *util, dp(dlo), dp(dhi)), "bocf_train_utility_range")
    np.testing.assert_allclose(dlo, lo, rtol=1e-13)
    np.testing.assert_allclose(dhi, hi, rtol=1e-13)
    u0d = _ffi.f64(u0 if given else dlo)
    G, P = np.empty(C), np.empty(C)
    _ffi.check(lib.bocf_expected_utility_constrained(h, *util, dp(u0d), rows.ctypes.data_as(c_int_p), nh, dp(G), dp(P), None),
               "bocf_expected_utility_constrained")
    eg, ep = np.abs(G - ref["G"]), np.abs(P - ref["P"])
    print("canned %s eta %g: |G| %.3g .. %.3g, P %.3g .. %.3g, scale %.3g, max abs err G %.3g, max rel err G %.3g, max rel err P %.3g"
          % (IDS[CASES.index(case)], eta, np.abs(ref["G"]).min(), np.abs(ref["G"]).max(), ref["P"].min(), ref["P"].max(), ref["scale"], eg.max(),
             np.max(eg / np.maximum(np.abs(ref["G"]), 1e-300)), np.max(ep / np.maximum(ref["P"], 1e-300))))
    assert np.all(np.isfinite(G)) and np.all(P >= 0) and np.all(P <= 1)
    np.testing.assert_allclose(G, ref["G"], rtol=1e-11, atol=1e-14 * ref["n_h"] * S * ref["scale"])
    np.testing.assert_allclose(P, ref["P"], rtol=1e-11, atol=0)
    # pof_out may be NULL; the gradient form is refused by name on a host-given posterior
    G2 = np.empty(C)
    _ffi.check(lib.bocf_expected_utility_constrained(h, *util, dp(u0d), rows.ctypes.data_as(c_int_p), nh, dp(G2), None, None),
               "bocf_expected_utility_constrained")
    np.testing.assert_array_equal(G2, G)
    assert lib.bocf_expected_utility_constrained(h, *util, dp(u0d), rows.ctypes.data_as(c_int_p), nh, dp(G2), None, dp(np.empty((C, 1)))) < 0
    msg = lib.bocf_last_error()
    assert b"bocf_expected_utility_constrained" in msg and b"host-given posterior" in msg
    ctx.close()


@pytest.mark.parametrize("N", [1, 63, 64, 65, 200])
def test_train_utility_range_against_numpy(N):
    rng = np.random.RandomState(50 + N)
    lib, ctx, dp = _ffi.load(), _ffi.Context(0), _ffi.dptr
    for kind, m, L in (("neg_sq_dist", 4, 3), ("neg_exp_cos", 3, 1), ("rosenbrock", 16, 2), ("linear", 9, 32)):
        mt = rng.uniform(-1.0, 1.0, size=(m, N))
        thetas, params = CR.utility_inputs(rng, kind, m, L)
        one = np.ones((m, 1))
        _ffi.check(lib.bocf_set_posterior(ctx.handle, m, 1, N, dp(one), dp(one), dp(_ffi.f64(mt))), "bocf_set_posterior")
        th, par = _ffi.f64(thetas), None if params is None else _ffi.f64(params)
        lo, hi = np.empty(L), np.empty(L)
        _ffi.check(lib.bocf_train_utility_range(ctx.handle, UTIL[kind], dp(par), 0 if par is None else par.size, dp(th), th.shape[1], L, dp(lo), dp(hi)),
                   "bocf_train_utility_range")
        want = _train_range(mt, thetas, kind, params)
        np.testing.assert_allclose(lo, want[0], rtol=1e-13)
        np.testing.assert_allclose(hi, want[1], rtol=1e-13)
    ctx.close()


# ---- through the model, against the restatement on the oracle's noiseless posterior -------------------------------------------------------
@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_values_against_the_restatement(case):
    inp, model, ref, _ = _case(case)
    S = inp["Z"].shape[1]
    G, P = _device(model, inp, inp["Xc"], inp["rows"])
    eg, ep = np.abs(G - ref["G"]), np.abs(P - ref["P"])
    print("ceu %s: |G| %.3g .. %.3g, P %.3g .. %.3g, scale %.3g, max abs err G %.3g, max rel err G %.3g, max abs err P %.3g"
          % (IDS[CASES.index(case)], np.abs(ref["G"]).min(), np.abs(ref["G"]).max(), ref["P"].min(), ref["P"].max(), ref["scale"], eg.max(),
             np.max(eg / np.maximum(np.abs(ref["G"]), 1e-300)), ep.max()))
    assert G.shape == P.shape == (case[6],) and np.all(np.isfinite(G))
    if not inp["given"]:
        model.set_hyperparameters(0)                                              # (the call left the model on its last hyper-sample)
        lo, hi = model.train_utility_range(UTIL[inp["kind"]], inp["params"], inp["thetas"])
        want = _train_range(inp["mts"][0], inp["thetas"], inp["kind"], inp["params"])
        np.testing.assert_allclose(lo, want[0], rtol=1e-6, atol=1e-9)
        np.testing.assert_allclose(hi, want[1], rtol=1e-6, atol=1e-9)
    np.testing.assert_allclose(G, ref["G"], rtol=1e-5, atol=1e-12 * ref["n_h"] * S * ref["scale"])
    np.testing.assert_allclose(P, ref["P"], rtol=1e-5, atol=1e-12)
    again = _device(model, inp, inp["Xc"], inp["rows"])                          # a second identical call: the same bits
    np.testing.assert_array_equal(again[0], G)
    np.testing.assert_array_equal(again[1], P)


@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_gradients_against_the_restatement(case):
    inp, model, _, ref = _case(case)
    X, rows = inp["Xc"][:NGRAD], inp["rows"][:NGRAD]
    S = inp["Z"].shape[1]
    G, P, dG = _device(model, inp, X, rows, grad=True)
    assert dG.shape == X.shape
    g = ref["dG"]
    print("ceu gradient %s: %d candidates, max abs err %.3g, gradient scale %.3g" % (IDS[CASES.index(case)], len(X), np.abs(dG - g).max(), np.abs(g).max()))
    np.testing.assert_allclose(G, ref["G"], rtol=1e-5, atol=1e-12 * ref["n_h"] * S * ref["scale"])
    np.testing.assert_allclose(P, ref["P"], rtol=1e-5, atol=1e-12)
    np.testing.assert_allclose(dG, g, rtol=1e-4, atol=1e-9 * max(1.0, np.abs(g).max()))
    value_only = _device(model, inp, X, rows)                                     # the value form and the gradient form: the same sums
    np.testing.assert_array_equal(value_only[0], G)
    np.testing.assert_array_equal(value_only[1], P)


@pytest.mark.parametrize("case", [BASE, _vary(H=2, N=100)], ids=["H1", "H2"])
def test_vacuous_constraints_give_the_plain_expected_utility(case):
    inp, model, _, _ = _case(case)
    oc = B.OutputConstraints(inp["A"], np.full(len(inp["b"]), 1e30), inp["eta"])
    nh = _n_hyps(inp["H"])
    G, P, dG = _device(model, inp, inp["Xc"][:NGRAD], inp["rows"][:NGRAD], grad=True, oc=oc)
    want, dwant = model.expected_utility(inp["Xc"][:NGRAD], "mc", inp["kind"], inp["thetas"], inp["rows"][:NGRAD], Z=inp["Z"], n_hyps=nh, grad=True,
                                         util_params=inp["params"])
    np.testing.assert_allclose(G, want, rtol=1e-12, atol=0)
    np.testing.assert_array_equal(P, np.ones(NGRAD))
    np.testing.assert_allclose(dG, dwant, rtol=1e-10, atol=1e-10 * np.abs(dwant).max())   # (B_j is summed in another association)


def test_batch_independence_bit_for_bit():
    case = _vary(C=257, N=64)
    inp, model, _, _ = _case(case)
    Xc, rows = inp["Xc"], inp["rows"]
    whole = _device(model, inp, Xc, rows, grad=True)
    for cut in (128, 101):
        a, b = _device(model, inp, Xc[:cut], rows[:cut], grad=True), _device(model, inp, Xc[cut:], rows[cut:], grad=True)
        for w, x, y in zip(whole, a, b):
            np.testing.assert_array_equal(np.concatenate([x, y]), w)
    model.set_option("chunk", 128)                                                # the predict pass's chunking: the same bits
    for w, x in zip(whole, _device(model, inp, Xc, rows, grad=True)):
        np.testing.assert_array_equal(x, w)
    model.set_option("chunk", 65536)


def test_state_is_left_alone_and_the_constraints_survive_model_changes():
    d, N, C = 3, 100, 60
    kinds = MIXED[:3]
    X, Y, var, ls, nz, Xc = K.problem(kinds, N, d, C, 5, noise=1e-4)
    model = _fixed_model(kinds, X, Y, var, ls, nz)
    rng = np.random.RandomState(0)
    support, prob = rng.uniform(-0.5, 0.5, size=(2, 3)), np.array([0.4, 0.6])
    W, Z = rng.normal(size=(25, 3)), rng.normal(size=(2, 25, 3))
    oc = B.OutputConstraints.bounds([None, -0.5, None], [0.4, None, None], eta=0.05)
    kind = _ffi.UTIL_NEG_SQ_DIST
    rows, u0 = np.arange(C) % 2, np.array([-3.0, -2.5])
    model.set_output_constraints(oc)
    acq = model.acq_mc(Xc, _ffi.ACQ_EI, kind, None, support, prob, W=W)          # the acquisition vector of these candidates stays resident
    top = model.select_topk(8)
    eu = model.expected_utility(Xc, "mc", "neg_sq_dist", support, rows, Z=Z, grad=True)
    cacq = model.acq_mc_constrained(Xc, kind, None, support, prob, W=W)
    best = model.feasible_best(kind, None, support)
    g2 = model.expected_utility_constrained(Xc, kind, support, rows, u0, Z, grad=True)
    model.acq_mc(Xc, _ffi.ACQ_EI, kind, None, support, prob, W=W)                # (a candidate upload forgets the acquisition vector: made again)
    lo, hi = model.train_utility_range(kind, None, support)
    g1 = model.expected_utility_constrained(None, kind, support, rows, u0, Z)       # X = None: the resident candidates
    model.expected_utility_constrained(None, kind, support, rows, u0, Z, grad=True)
    np.testing.assert_array_equal(g1[0], g2[0])
    assert np.all(lo <= hi)
    assert model._resident.constraints == oc.key()
    # the acquisition vector (no acquisition call in between), W, bocf_expected_utility and the constrained acquisition answer as before
    for x, y in zip(top, model.select_topk(8)):
        np.testing.assert_array_equal(x, y)
    lib, h, dp = _ffi.load(), model._context().handle, _ffi.dptr
    out = np.empty(C)
    assert lib.bocf_acq_mc(h, _ffi.ACQ_EI, kind, None, 0, dp(_ffi.f64(support)), 3, dp(_ffi.f64(prob)), 2, dp(out)) == 0     # (W as resident)
    np.testing.assert_array_equal(out, acq)
    for x, y in zip(eu, model.expected_utility(Xc, "mc", "neg_sq_dist", support, rows, Z=Z, grad=True)):
        np.testing.assert_array_equal(x, y)
    np.testing.assert_array_equal(model.acq_mc_constrained(Xc, kind, None, support, prob, W=W), cacq)
    np.testing.assert_array_equal(model.feasible_best(kind, None, support)[0], best[0])
    # new targets, an appended observation and a refit: the constraints stay resident -- the C call works without sending them again
    th, G, P = _ffi.f64(support), np.empty(C), np.empty(C)
    r32 = rows.astype(np.int32)
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
        model.set_eu_samples(Z)
        assert lib.bocf_set_candidates(h, dp(_ffi.f64(Xc)), C) == 0
        assert lib.bocf_expected_utility_constrained(h, kind, None, 0, dp(th), 3, 2, dp(u0), r32.ctypes.data_as(c_int_p), 2, dp(G), dp(P), None) == 0, \
            (change, lib.bocf_last_error())
        la = K.LookAhead.fit(kinds, X, Y, var, ls, nz)
        post = CE.posterior_noiseless(la, Xc)
        ref = CE.constrained_eu_hyper([post[0]], [post[1]], Z, support, rows, u0, "neg_sq_dist", None, oc.A, oc.b, oc.eta, 2)
        np.testing.assert_allclose(G, ref["G"], rtol=1e-5, atol=1e-12 * 25 * ref["scale"])
        np.testing.assert_allclose(P, ref["P"], rtol=1e-5, atol=1e-12)
    model.set_output_constraints(None)
    with pytest.raises(RuntimeError, match="constraints"):
        model.expected_utility_constrained(Xc, kind, support, rows, u0, Z)
    with pytest.raises(IndexError):
        hm = _hyper_model(kinds, X, Y, var, ls, nz, 2)
        hm.set_output_constraints(oc)
        hm.expected_utility_constrained(Xc, kind, support, rows, u0, Z, n_hyps=3)


def test_every_refusal_names_its_entry_point():
    d, N, C = 2, 50, 20
    kinds = MIXED[:3]
    X, Y, var, ls, nz, Xc = K.problem(kinds, N, d, C, 9, noise=1e-4)
    lib, dp = _ffi.load(), _ffi.dptr
    A, b, eta, th, out = np.ones((2, 3)), np.zeros(2), np.full(2, 0.1), np.zeros((2, 3)), np.empty(C)
    rows, u0 = (np.arange(C) % 2).astype(np.int32), np.array([-1.0, -2.0])
    who = "bocf_expected_utility_constrained"

    def bad(rc, name, text):
        msg = lib.bocf_last_error()
        assert rc < 0 and name.encode() in msg and text.encode() in msg, (rc, msg, text)
    fresh = _ffi.Context(0)
    assert lib.bocf_set_output_constraints(fresh.handle, dp(A), dp(b), dp(eta), 2, 3) == 0
    bad(lib.bocf_expected_utility_constrained(fresh.handle, 1, None, 0, dp(th), 3, 2, dp(u0), rows.ctypes.data_as(c_int_p), 1, dp(out), None, None), who,
        "model not fitted")
    bad(lib.bocf_train_utility_range(fresh.handle, 1, None, 0, dp(th), 3, 2, dp(out), dp(out)), "bocf_train_utility_range", "model not fitted")
    fresh.close()
    model = _fixed_model(kinds, X, Y, var, ls, nz)
    model._ensure_fitted()
    h = model._context().handle

    def call(util=_ffi.UTIL_NEG_SQ_DIST, theta=th, tdim=3, L=2, u=u0, r=rows, nh=1, val=out, g=None):
        return lib.bocf_expected_utility_constrained(h, util, None, 0, dp(theta), tdim, L, dp(u), None if r is None else r.ctypes.data_as(c_int_p), nh,
                                                     dp(val), None, dp(g))
    assert lib.bocf_set_candidates(h, dp(_ffi.f64(Xc)), C) == 0
    bad(call(), who, "no output constraints")
    assert lib.bocf_train_utility_range(h, 1, None, 0, dp(th), 3, 2, dp(np.empty(2)), dp(np.empty(2))) == 0          # needs no constraints
    bad(lib.bocf_train_utility_range(h, 1, None, 0, dp(th), 3, 2, None, dp(np.empty(2))), "bocf_train_utility_range", "null")
    bad(lib.bocf_train_utility_range(h, _ffi.UTIL_PROGRAM, None, 0, dp(th), 3, 2, dp(np.empty(2)), dp(np.empty(2))), "bocf_train_utility_range",
        "BOCF_UTIL_PROGRAM")
    assert lib.bocf_set_output_constraints(h, dp(A[:, :2].copy()), dp(b), dp(eta), 2, 2) < 0
    assert lib.bocf_set_output_constraints(h, dp(A), dp(b), dp(eta), 2, 3) == 0
    bad(call(), who, "no Monte-Carlo samples")
    Z = np.random.RandomState(2).normal(size=(2, 4, 3))
    model.set_eu_samples(Z[:1])
    bad(call(), who, "fewer Monte-Carlo sample blocks")
    model.set_eu_samples(Z)
    bad(call(util=_ffi.UTIL_PROGRAM), who, "constrained expected utility does not take a utility program (BOCF_UTIL_PROGRAM)")
    bad(call(util=7), who, "unknown utility kind")
    bad(call(L=0), who, "L out of range")
    bad(call(theta=None), who, "theta")
    bad(call(tdim=2), who, "theta_dim must equal m")
    bad(call(util=_ffi.UTIL_ROSENBROCK, tdim=1), who, "even m")
    bad(call(u=None), who, "u_infeasible is null")
    bad(call(u=np.array([-1.0, np.nan])), who, "non-finite")
    bad(call(u=np.array([np.inf, -1.0])), who, "non-finite")
    bad(call(nh=0), who, "n_hyps must be >= 1")
    bad(call(val=None), who, "null output")
    bad(call(r=None), who, "null output")
    r2 = rows.copy()
    r2[-1] = 2
    bad(call(r=r2), who, "row_param out of range")
    r2[-1] = -1
    bad(call(r=r2), who, "row_param out of range")
    assert call() == 0 and call(g=np.empty((C, d))) == 0 and call(nh=7) == 0
    assert lib.bocf_set_candidates(h, dp(_ffi.f64(Xc)), 0) == 0 and call(val=None, r=None) == 0          # no candidate: nothing to do
    assert lib.bocf_set_candidates(h, dp(_ffi.f64(Xc)), C) == 0
    # the hyper-sample layout changed under resident constraints and samples
    model.set_option("hyper_samples", 3)
    bad(call(), who, "another m")
    model.set_option("hyper_samples", 1)                  # (a change of the layout forgets the device's Monte-Carlo samples)
    bad(call(), who, "no Monte-Carlo samples")
    assert lib.bocf_set_eu_samples(h, dp(_ffi.f64(Z)), 2, 4) == 0 and call() == 0
    # more hyper-samples than are resident; Z for another m
    hm = _hyper_model(kinds, X, Y, var, ls, nz, 2)
    hm.set_output_constraints(B.OutputConstraints(A, b, eta))
    hm.set_eu_samples(Z)
    hh = hm._context().handle
    assert lib.bocf_set_candidates(hh, dp(_ffi.f64(Xc)), C) == 0
    rc = lib.bocf_expected_utility_constrained(hh, 1, None, 0, dp(th), 3, 2, dp(u0), rows.ctypes.data_as(c_int_p), 3, dp(out), None, None)
    bad(rc, who, "n_hyps exceeds")
    assert lib.bocf_expected_utility_constrained(hh, 1, None, 0, dp(th), 3, 2, dp(u0), rows.ctypes.data_as(c_int_p), 2, dp(out), None, None) == 0


# ---- end to end ---------------------------------------------------------------------------------------------------------------------------
def _toy():
    d, m = 2, 2
    space = B.Design_space([{'name': 'x', 'type': 'continuous', 'domain': (0, 1), 'dimensionality': d}])
    f = [lambda x: np.sin(3 * x[:, :1]) * x[:, 1:2] + x[:, :1] ** 2, lambda x: np.cos(2 * x[:, 1:2]) + 0.5 * x[:, :1]]
    model = B.multi_outputGP(m, kernel=[B.kern.RBF(d, variance=1.0, lengthscale=0.3, ARD=True) for _ in range(m)], noise_var=[1e-4] * m, fixed_hyps=True)
    U = B.Utility(parameter_dist=B.ParameterDistribution(support=np.array([[0.9, 0.9], [0.5, 1.2]]), prob_dist=np.array([0.5, 0.5])), device="neg_sq_dist")
    oc = B.OutputConstraints.bounds([None, None], [0.6, None], eta=0.02)         # y_0 <= 0.6 cuts off what the first parameter aims at
    return space, f, model, U, oc


def test_the_recommendation_step_with_constraints_against_the_restatement():
    """current_marginal_argmaxes on the device against the same call with evaluator= the restatement over the model's own noiseless
    posterior (its public predict_noiseless and gradients, as tests/test_gpu_recommend.py compares; those go through the small-batch
    path for the 48 anchors and the chunked pass for the 400 starts, which agree to ~1e-12): arguments to 1e-4, values to 1e-6."""
    space, f, model, U, oc = _toy()
    np.random.seed(43)
    X0 = np.random.uniform(size=(12, 2))
    model.updateModel(X0, [fj(X0) for fj in f])
    support = U.parameter_dist.support
    kw = dict(n_hyps=2, n_starting=200, n_anchor=24, constraints=oc)
    np.random.seed(7)
    info = {}
    x_dev, v_dev = B.current_marginal_argmaxes(model, space, U, support, info=info, **kw)
    u0 = info["u_infeasible"]
    mt = model.posterior_mean_at_evaluated_points()
    np.testing.assert_allclose(u0, _train_range(mt, support, "neg_sq_dist", None)[0], rtol=1e-12)
    np.random.seed(7)
    ref_info = {}
    x_ref, v_ref = B.current_marginal_argmaxes(model, space, U, support, evaluator=CE.restated_factory(model, "neg_sq_dist", 2), info=ref_info,
                                               infeasible_utility=u0, **kw)
    np.testing.assert_array_equal(info["designs"], ref_info["designs"])
    np.testing.assert_array_equal(info["Z"], ref_info["Z"])
    print("constrained recommendation: x %s against %s, values %s against %s, pof %s" % (x_dev.tolist(), x_ref.tolist(), v_dev, v_ref, info["pof"]))
    np.testing.assert_allclose(x_dev, x_ref, rtol=0, atol=1e-4)
    np.testing.assert_allclose(v_dev, v_ref, rtol=1e-6)
    np.testing.assert_allclose(info["pof"], ref_info["pof"], rtol=1e-5, atol=1e-9)
    mean = model.predict_noiseless(x_dev)[0]
    assert np.all(oc.feasible(mean)) and np.all(info["pof"] > 0.5)
    # without constraints the first parameter's recommendation is infeasible: the constraint decides
    np.random.seed(7)
    x_free, _ = B.current_marginal_argmaxes(model, space, U, support, n_hyps=2)
    assert not oc.feasible(model.predict_noiseless(x_free[:1])[0][:, 0])


def test_cbo_with_constraints_records_finite_values_and_pof():
    space, f, model, U, oc = _toy()
    np.random.seed(44)
    opt = B.AcquisitionOptimizer(space, optimizer='lbfgs', n_starting=200, n_anchor=8)
    acq = B.uEI_constrained(model, space, optimizer=opt, utility=U, constraints=oc)
    X0 = np.random.uniform(size=(10, 2))
    bo = B.CBO(model, space, B.MultiObjective(f, noise_var=[1e-4, 1e-4]), acq, B.Sequential(acq), X0, constraints=oc)
    bo.run_optimization(max_iter=2)
    assert bo.X.shape == (12, 2) and len(bo.historical_optimal_values) == 2 and np.all(np.isfinite(bo.historical_optimal_values))
    rec = bo.last_recommendation
    assert rec["pof"].shape == (2,) and np.all(np.isfinite(rec["pof"])) and np.all(rec["pof"] >= 0) and np.all(rec["pof"] <= 1)
    assert np.all(np.isfinite(rec["u_infeasible"])) and bo.current_argmax.shape == (1, 2)
