"""Utility programs on the device (csrc/util_prog.hip): the interpreter against the NumPy interpreter of the same blob value by value,
the traced program against the compiled-in utility of the same expression and against the host fallback with the user's own
func / dfunc, the recommendation step, the batch / run / program-replacement invariants, the loud errors and the Thompson batch.
Run on the MI355X box:  python -m pytest tests -m gpu"""
import ctypes
import warnings

import numpy as np
import pytest

from bocf_amd import utility_program as UP
from oracle import cpu_ref as R

pytestmark = pytest.mark.gpu
PI = np.pi


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


# ---- utilities: each works on y (m,) of nodes and on y (m, n) of floats; *_terms gives the additive terms of U for the error scale
def neg_sq_dist(t, y):
    return -np.sum(np.square((y.transpose() - t).transpose()), axis=0)


def linear(t, y):
    return np.dot(t, y)


def neg_sum_exp(t, y):
    return np.sum(-np.exp(y), axis=0)


def make_neg_exp_cos(c):
    c = np.asarray(c, dtype=float)

    def terms(t, y):
        return (c * (np.exp(-y / PI) * np.cos(PI * y)).T).T

    def U(t, y):
        return -np.sum(terms(t, y), axis=0)
    return U, terms


def rosenbrock(a, y):
    h = y.shape[0] // 2
    val = 0
    for j in range(h):
        val -= (a[0] - y[j]) ** 2 + 100 * y[j + h] ** 2
    return val


def abs15(t, y):                                            # the callable of tests/test_host_cpu.py:316 and its dfunc
    return -np.sum(np.abs((np.asarray(y).T - t).T) ** 1.5, axis=0)


def d_abs15(t, y):
    return -1.5 * np.sign((np.asarray(y).T - t).T) * np.abs((np.asarray(y).T - t).T) ** 0.5


def tanh_ratio(t, y):
    return -np.sum(np.tanh(y) ** 2 / (1 + y ** 2), axis=0)


def _dist(B, support, prob=None):
    support = np.atleast_2d(support)
    return B.ParameterDistribution(support=support, prob_dist=np.full(len(support), 1.0 / len(support)) if prob is None else prob)


# ---------------------------------------------------------------------------------------------
# 1. the device interpreter against the NumPy interpreter, value by value: bocf_thompson_select returns u(p, c) itself
def _max_size_program(m):
    """A blob built directly at the maximum slot and instruction counts: r_i = r_{i-1} / 2 (even i) or r_{i-1} + y_{i mod m} (odd i), the
    destination walking through all slots; + and x only, bounded values."""
    n, slots = UP.MAX_INSTR, UP.MAX_SLOTS
    code = [(UP.OP["MUL"], 0, UP.K_INPUT << 14 | 0, UP.K_CONST << 14 | 0)]
    for i in range(1, n):
        prev = UP.K_SLOT << 14 | (i - 1) % slots
        if i % 2 == 0:
            code.append((UP.OP["MUL"], i % slots, prev, UP.K_CONST << 14 | 0))
        else:
            code.append((UP.OP["ADD"], i % slots, prev, UP.K_INPUT << 14 | i % m))
    last = (n - 1) % slots
    return UP.Program(m, 1, slots, code, last, code, [last] + [(last - 1 - j) % slots for j in range(m)], [0.5])


@pytest.mark.parametrize("m", [1, 3, 4, 9, 16])
def test_interpreter_equals_numpy_value_by_value(B, m):
    F = B._ffi
    N, d, C, P = 32, 2, 48, 3
    p = R.synthetic_problem(N, d, m, C, 4, 31 + m, noise=1e-4)
    model = _model(B, "rbf", p["X"], p["Y"], p["variances"], p["lengthscales"], p["noise"])
    model._set_candidates(p["Xc"])
    rng = np.random.RandomState(m)
    samples, _ = model._posterior_samples(0, rng.normal(size=(m, C, P)))          # samples_out: (m, C, P), the inputs of every u(p, c)
    lib, h = F.load(), model._context().handle
    c = 1.0 + 0.5 * np.arange(m)
    nec, nec_terms = make_neg_exp_cos(c)
    # (name, program, theta_dim, additive terms for the error scale or None = bit for bit)
    progs = [("neg_sq_dist", UP.trace(neg_sq_dist, m, m), m, None),
             ("y0", UP.trace(lambda t, y: y[0], m, 1), 1, None),
             ("max_size", _max_size_program(m), 1, None),
             ("neg_sum_exp", UP.trace(neg_sum_exp, m, 1), 1, lambda t, y: np.exp(y)),
             ("neg_exp_cos", UP.trace(nec, m, 1), 1, nec_terms),
             ("tanh_ratio", UP.trace(tanh_ratio, m, 1), 1, lambda t, y: np.tanh(y) ** 2 / (1 + y ** 2)),
             ("abs15", UP.trace(abs15, m, m), m, lambda t, y: np.abs((y.T - t).T) ** 1.5)]
    if m == 4:
        progs.append(("rosenbrock", UP.trace(rosenbrock, m, 1), 1, None))
    assert len(progs[1][1].val_code) == 1 and len(progs[2][1].val_code) == UP.MAX_INSTR and progs[2][1].n_slots == UP.MAX_SLOTS
    for name, prog, td, terms in progs:
        blob = prog.to_bytes()
        assert lib.bocf_check_utility_program(blob, len(blob), m, td) == 0, lib.bocf_last_error()
        model.set_utility_program(blob)
        theta = F.f64(rng.uniform(-1.0, 1.0, size=(P, td)))                       # P paths with different theta
        idx, val = np.empty((P, C), dtype=np.int64), np.empty((P, C))
        F.check(lib.bocf_thompson_select(h, F.UTIL_PROGRAM, None, 0, F.dptr(theta), td, C, idx.ctypes.data_as(F._c_ll_p), F.dptr(val)),
                "bocf_thompson_select")
        for q in range(P):
            assert sorted(idx[q].tolist()) == list(range(C)), name                # k = C: every candidate once
            want = prog.value(theta[q], samples[:, :, q])
            got = np.empty(C)
            got[idx[q]] = val[q]
            err = np.abs(got - want)
            print("%s m=%d path %d: max |device - numpy| = %.3e" % (name, m, q, err.max()))
            if terms is None:
                assert np.array_equal(got, want), (name, m, q, err.max())         # + - x: bit for bit
            else:
                scale = np.sum(np.abs(terms(theta[q], samples[:, :, q])), axis=0)
                assert np.all(err <= 1e-12 * scale), (name, m, q, (err / scale).max())


# ---------------------------------------------------------------------------------------------
# 2. the traced program against the compiled-in kind of the same expression (cases and inputs of test_acquisitions_vs_oracle)
def _check_ei_pi_grad(B, model, Xc, W, S, U_ref, U_prog, n_grad=5, ref_warns=False):
    def run(U, cls, grad, X=None):
        acq = cls(model, None, utility=U)
        acq.W_samples = W
        with warnings.catch_warnings():
            if U is U_prog or not ref_warns:
                warnings.simplefilter("error")                # the program path (and a compiled-in kind) must not warn
            else:
                warnings.simplefilter("ignore")
            return acq._compute_acq_withGradients(Xc[:n_grad] if X is None else X) if grad else acq._compute_acq(Xc)
    a, r = run(U_prog, B.uEI_noiseless, False), run(U_ref, B.uEI_noiseless, False)
    print("EI: max |program - reference| = %.3e (max |reference| %.3e)" % (np.abs(a - r).max(), np.abs(r).max()))
    np.testing.assert_allclose(a, r, rtol=1e-5, atol=1e-9)
    a, r = run(U_prog, B.uPI, False), run(U_ref, B.uPI, False)
    print("PI: share differing %.4f, max difference %.3e" % (np.mean(np.abs(a - r) > 1e-12), np.abs(a - r).max()))
    assert np.mean(np.abs(a - r) > 1e-12) <= 0.01
    assert np.abs(a - r).max() <= 1.0 / S + 1e-12
    (a, da), (r, dr) = run(U_prog, B.uEI_noiseless, True), run(U_ref, B.uEI_noiseless, True)
    print("EI gradient: max |program - reference| = %.3e (max |reference| %.3e)" % (np.abs(da - dr).max(), np.abs(dr).max()))
    np.testing.assert_allclose(a, r, rtol=1e-5, atol=1e-9)
    np.testing.assert_allclose(da, dr, rtol=1e-4, atol=1e-8)
    # (the first candidates may all have EI = 0 and a zero gradient: the same bounds on the candidates with the largest EI as well)
    top = Xc[np.argsort(-run(U_ref, B.uEI_noiseless, False)[:, 0], kind="stable")[:n_grad]]
    (a, da), (r, dr) = run(U_prog, B.uEI_noiseless, True, top), run(U_ref, B.uEI_noiseless, True, top)
    print("EI gradient, largest EI: max |program - reference| = %.3e (max |reference| %.3e)" % (np.abs(da - dr).max(), np.abs(dr).max()))
    assert np.abs(dr).max() > 0
    np.testing.assert_allclose(a, r, rtol=1e-5, atol=1e-9)
    np.testing.assert_allclose(da, dr, rtol=1e-4, atol=1e-8)


@pytest.mark.parametrize("util,m", [("neg_sq_dist", 3), ("neg_sum_exp", 3), ("neg_exp_cos", 3), ("rosenbrock", 4), ("linear", 3)])
def test_traced_program_equals_the_builtin_kind(B, util, m):
    N, d, C, S = 150, 3, 333, 50
    p = R.synthetic_problem(N, d, m, C, S, 99, noise=1e-4)
    model = _model(B, "matern52", p["X"], p["Y"], p["variances"], p["lengthscales"], p["noise"])
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
    func = {"neg_sq_dist": neg_sq_dist, "linear": linear, "neg_sum_exp": neg_sum_exp, "rosenbrock": rosenbrock,
            "neg_exp_cos": make_neg_exp_cos([1.0, 2.0, 5.0])[0]}[util]
    U_ref = B.Utility(parameter_dist=_dist(B, support, prob), device=util, device_params=params)
    U_prog = B.Utility(func=func, parameter_dist=_dist(B, support, prob), device="program")
    _check_ei_pi_grad(B, model, p["Xc"], p["W"], S, U_ref, U_prog)


# ---------------------------------------------------------------------------------------------
# 3. against the host fallback with the user's own func / dfunc
@pytest.mark.parametrize("C,S", [(64, 32), (64, 70), (5, 32)])     # S = 70: two ragged lane strides; C = 5: one partial workgroup
def test_program_equals_the_host_fallback(B, C, S):
    N, d, m = 24, 3, 3
    p = R.synthetic_problem(N, d, m, C, S, 7, noise=1e-4)
    model = _model(B, "se", p["X"], p["Y"], p["variances"], p["lengthscales"], p["noise"])
    theta, prob = np.array([[0.3, -0.1, 0.2], [0.0, 0.4, -0.3]]), np.array([0.25, 0.75])
    U_host = B.Utility(func=abs15, dfunc=d_abs15, parameter_dist=_dist(B, theta, prob))
    U_prog = B.Utility(func=abs15, parameter_dist=_dist(B, theta, prob), device="program")
    acq = B.uEI_noiseless(model, None, utility=U_host)
    acq.W_samples = p["W"]
    with pytest.warns(RuntimeWarning, match="HOST"):          # device=None: the warned host path, as before
        acq._compute_acq(p["Xc"])
    _check_ei_pi_grad(B, model, p["Xc"], p["W"], S, U_host, U_prog, ref_warns=True)


# ---------------------------------------------------------------------------------------------
# 4. the recommendation step: bocf_expected_utility in Monte-Carlo mode
def test_expected_utility_mc(B):
    N, d, m, C, S, L = 64, 2, 3, 10, 40, 2
    p = R.synthetic_problem(N, d, m, C, S, 17, noise=1e-4)
    model = _model(B, "rbf", p["X"], p["Y"], p["variances"], p["lengthscales"], p["noise"])
    rng = np.random.RandomState(2)
    Z = rng.normal(size=(L, S, m))
    rows = np.arange(C) % L                                   # rows alternating between the two parameters
    thetas = np.ones((L, 1))
    U_ref = B.Utility(parameter_dist=_dist(B, thetas), device="neg_sum_exp")
    U_prog = B.Utility(func=neg_sum_exp, parameter_dist=_dist(B, thetas), device="program")
    v, g = model.expected_utility(p["Xc"], "mc", U_prog, thetas, rows, Z=Z, n_hyps=1, grad=True)
    rv, rg = model.expected_utility(p["Xc"], "mc", U_ref, thetas, rows, Z=Z, n_hyps=1, grad=True)
    print("EU: max |program - builtin| value %.3e gradient %.3e" % (np.abs(v - rv).max(), np.abs(g - rg).max()))
    np.testing.assert_allclose(v, rv, rtol=1e-5, atol=1e-9)
    np.testing.assert_allclose(g, rg, rtol=1e-4, atol=1e-8)
    np.testing.assert_array_equal(model.expected_utility(p["Xc"], "mc", U_prog, thetas, rows, Z=Z, n_hyps=1), v)      # value-only form
    h = 1e-6
    fd = np.empty_like(g)
    for q in range(d):
        Xp, Xm = p["Xc"].copy(), p["Xc"].copy()
        Xp[:, q] += h
        Xm[:, q] -= h
        fd[:, q] = (model.expected_utility(Xp, "mc", U_prog, thetas, rows, Z=Z, n_hyps=1) -
                    model.expected_utility(Xm, "mc", U_prog, thetas, rows, Z=Z, n_hyps=1)) / (2 * h)
    print("EU: max relative |gradient - central differences| = %.3e" % (np.abs(g - fd) / np.abs(fd)).max())
    np.testing.assert_allclose(g, fd, rtol=1e-4)
    # the recommendation step takes its Monte-Carlo device branch for a program utility (no closed form, no host warning)
    from bocf_amd import recommend
    with warnings.catch_warnings():
        warnings.simplefilter("error")
        ev = recommend.make_evaluator(model, "mc", U_prog, thetas, None, Z, 1)
    np.testing.assert_array_equal(ev(p["Xc"], rows, False)[0], v)


# ---------------------------------------------------------------------------------------------
# 5. invariants
def test_invariants(B):
    N, d, m, C, S = 24, 3, 3, 64, 32
    p = R.synthetic_problem(N, d, m, C, S, 7, noise=1e-4)
    theta, prob = np.array([[0.3, -0.1, 0.2], [0.0, 0.4, -0.3]]), np.array([0.25, 0.75])

    def fresh():
        return _model(B, "se", p["X"], p["Y"], p["variances"], p["lengthscales"], p["noise"])

    def ei(model, U, X, grad=False):
        acq = B.uEI_noiseless(model, None, utility=U)
        acq.W_samples = p["W"]
        return acq._compute_acq_withGradients(X) if grad else acq._compute_acq(X)
    model = fresh()
    U_a = B.Utility(func=abs15, parameter_dist=_dist(B, theta, prob), device="program")
    U_b = B.Utility(func=lambda t, y: 2.0 * abs15(t, y), parameter_dist=_dist(B, theta, prob), device="program")     # B = 2 A, same theta
    U_nsd = B.Utility(parameter_dist=_dist(B, theta, prob), device="neg_sq_dist")
    whole = ei(model, U_a, p["Xc"])
    gw, dgw = ei(model, U_a, p["Xc"], grad=True)
    np.testing.assert_array_equal(np.concatenate((ei(model, U_a, p["Xc"][:C // 2]), ei(model, U_a, p["Xc"][C // 2:]))), whole)   # halves == whole
    g1, dg1 = ei(model, U_a, p["Xc"][:C // 2], grad=True)
    g2, dg2 = ei(model, U_a, p["Xc"][C // 2:], grad=True)
    np.testing.assert_array_equal(np.concatenate((g1, g2)), gw)
    np.testing.assert_array_equal(np.concatenate((dg1, dg2)), dgw)
    np.testing.assert_array_equal(ei(model, U_a, p["Xc"]), whole)                      # two runs are bit-identical
    np.testing.assert_array_equal(ei(model, U_a, p["Xc"], grad=True)[1], dgw)
    assert np.abs(whole).max() > 0 and np.abs(dgw).max() > 0
    # replacing the program with theta unchanged replaces best_l: B after A equals B on a fresh context -- and, a factor of two being
    # exact in every operation of U, best and the hinge, exactly twice A's value (with A's best it would not be)
    after_a = ei(model, U_b, p["Xc"])
    np.testing.assert_array_equal(after_a, ei(fresh(), U_b, p["Xc"]))
    np.testing.assert_array_equal(after_a, 2.0 * whole)
    # a compiled-in kind and the program on one context: each its own result, whatever ran before
    r_nsd = ei(fresh(), U_nsd, p["Xc"])
    np.testing.assert_array_equal(ei(model, U_nsd, p["Xc"]), r_nsd)
    np.testing.assert_array_equal(ei(model, U_a, p["Xc"]), whole)
    np.testing.assert_array_equal(ei(model, U_nsd, p["Xc"]), r_nsd)
    np.testing.assert_array_equal(ei(model, U_b, p["Xc"]), after_a)


# ---------------------------------------------------------------------------------------------
# 6. errors are loud and precede any launch
def test_errors(B):
    F = B._ffi
    N, d, m, C, S = 24, 3, 3, 8, 16
    p = R.synthetic_problem(N, d, m, C, S, 7, noise=1e-4)
    model = _model(B, "se", p["X"], p["Y"], p["variances"], p["lengthscales"], p["noise"])
    lib, h = F.load(), model._context().handle
    model.set_mc_samples(p["W"])
    model._set_candidates(p["Xc"])
    theta = F.f64(np.array([[0.3, -0.1, 0.2]]))
    out, gout = np.empty(C), np.empty((C, d))

    def bad(rc, *words):
        err = lib.bocf_last_error().decode()
        assert rc < 0 and all(w in err for w in words), (rc, err)
    # the program kind with no program staged
    bad(lib.bocf_acq_mc(h, F.ACQ_EI, F.UTIL_PROGRAM, None, 0, F.dptr(theta), m, None, 1, F.dptr(out)), "bocf_acq_mc", "no utility program")
    bad(lib.bocf_acq_mc_grad(h, F.UTIL_PROGRAM, None, 0, F.dptr(theta), m, None, 1, F.dptr(out), F.dptr(gout)), "bocf_acq_mc_grad", "no utility program")
    # wrong m, wrong theta_dim, util_params given
    two = UP.trace(abs15, 2, 2).to_bytes()
    assert lib.bocf_set_utility_program(h, two, len(two)) == 0
    bad(lib.bocf_acq_mc(h, F.ACQ_EI, F.UTIL_PROGRAM, None, 0, F.dptr(theta), 2, None, 1, F.dptr(out)), "bocf_acq_mc", "m = 2")
    three = UP.trace(abs15, m, m).to_bytes()
    assert lib.bocf_set_utility_program(h, three, len(three)) == 0
    bad(lib.bocf_acq_mc(h, F.ACQ_EI, F.UTIL_PROGRAM, None, 0, F.dptr(theta), 1, None, 1, F.dptr(out)), "bocf_acq_mc", "theta_dim")
    bad(lib.bocf_acq_mc(h, F.ACQ_EI, F.UTIL_PROGRAM, F.dptr(theta), 3, F.dptr(theta), m, None, 1, F.dptr(out)), "bocf_acq_mc", "util_params")
    assert lib.bocf_acq_mc(h, F.ACQ_EI, F.UTIL_PROGRAM, None, 0, F.dptr(theta), m, None, 1, F.dptr(out)) == 0        # and the right call runs
    # a rejected blob never replaces the resident program
    bad(lib.bocf_set_utility_program(h, three[:-8], len(three) - 8), "bocf_set_utility_program", "truncated")
    again = np.empty(C)
    assert lib.bocf_acq_mc(h, F.ACQ_EI, F.UTIL_PROGRAM, None, 0, F.dptr(theta), m, None, 1, F.dptr(again)) == 0
    np.testing.assert_array_equal(again, out)
    # no closed form, no knowledge gradient
    rows = np.zeros(C, dtype=np.int32)
    bad(lib.bocf_expected_utility(h, F.EU_CLOSED, F.UTIL_PROGRAM, None, 0, F.dptr(theta), m, 1, rows.ctypes.data_as(ctypes.POINTER(ctypes.c_int)), 1,
                                  F.dptr(out), None), "bocf_expected_utility", "closed-form")
    Zf = F.f64(np.zeros((2, m)))
    bad(lib.bocf_acq_kg(h, F.EU_MC, F.UTIL_PROGRAM, None, 0, F.dptr(theta), m, None, 1, F.dptr(Zf), 2, F.dptr(out), None), "bocf_acq_kg",
        "knowledge gradient")
    U = B.Utility(func=abs15, parameter_dist=_dist(B, theta), device="program")
    with pytest.raises(NotImplementedError):
        B.uKG(model, None, utility=U)._compute_acq(p["Xc"])
    # an explicit request never falls back to the host: a callable that cannot be traced raises from the acquisition
    U_bad = B.Utility(func=lambda t, y: np.sum(np.maximum(y, 0.0)), parameter_dist=_dist(B, theta), device="program")
    with pytest.raises(UP.TraceError):
        B.uEI_noiseless(model, None, utility=U_bad)._compute_acq(p["Xc"])


# ---------------------------------------------------------------------------------------------
# 7. CompositeThompsonBatch with a program utility
def test_composite_thompson_batch(B):
    np.random.seed(5)
    d, m, q, N = 2, 2, 4, 48
    space = B.Design_space([{'name': 'x', 'type': 'continuous', 'domain': (0, 1), 'dimensionality': d}])
    X = np.random.uniform(size=(N, d))
    Y = [np.sin(3 * X[:, :1]) * X[:, 1:2] + X[:, :1] ** 2, np.cos(2 * X[:, 1:2]) + 0.5 * X[:, :1]]
    model = B.multi_outputGP(m, kernel=[B.kern.RBF(d, variance=1.0, lengthscale=0.3, ARD=True) for _ in range(m)], noise_var=[1e-4] * m,
                             fixed_hyps=True)
    model.updateModel(X, Y)
    U = B.Utility(func=abs15, parameter_dist=_dist(B, np.array([[0.5, 0.2], [0.1, 0.9]])), device="program")
    acq = B.uEI_noiseless(model, space, optimizer=B.AcquisitionOptimizer(space, optimizer='lbfgs', n_starting=64, n_anchor=2), utility=U)
    with warnings.catch_warnings():
        warnings.simplefilter("error", RuntimeWarning)
        batch = B.CompositeThompsonBatch(acq, q, n_candidates=256).compute_batch()
    assert batch.shape == (q, d) and len({tuple(r) for r in batch}) == q
    assert np.all(batch >= 0.0) and np.all(batch <= 1.0)
