"""Feasibility-aware recommendation, CPU side: the NumPy restatement tests/ceu_ref.py -- vacuous constraints against
the oracle's plain Monte-Carlo expected utility, the indicator limit, the affine dependence on u0, its gradient against central
differences of its own value --, the decision property on an oracle posterior, the surface (header, exports, keywords, RNG order, the
calls an unconstrained step makes) and the argument checks of the two entry points through tests/ceu_args_driver.cpp, built once as it
is and once with AddressSanitizer and UndefinedBehaviorSanitizer."""
import ctypes
import inspect
import os
import re
import subprocess
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import ceu_ref as CE  # noqa: E402
import constrained_ref as CR  # noqa: E402
import kg_ref as K  # noqa: E402
import test_model_calls_cpu as MC  # noqa: E402

import bocf_amd as B  # noqa: E402
from bocf_amd import _ffi  # noqa: E402
from bocf_amd import recommend as REC  # noqa: E402
from oracle import cpu_ref as O  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CLANG = "/opt/rocm/lib/llvm/bin/clang++"
ENTRY_POINTS = ["bocf_train_utility_range", "bocf_expected_utility_constrained"]
UTILS = ["linear", "neg_sq_dist", "neg_sum_exp", "neg_exp_cos", "rosenbrock"]


def _small(kind, seed=3, N=14, d=2, m=2, S=40, L=3, n=12, Kc=2, eta=0.05):
    kinds = ["se", "matern52", "rbf", "matern32"][:m]
    X, Y, var, ls, nz, Xc = K.problem(kinds, N, d, n, seed, noise=1e-4)
    la = K.LookAhead.fit(kinds, X, Y, var, ls, nz)
    rng = np.random.RandomState(200 + seed)
    Z = rng.normal(size=(L, S, m))
    thetas, params = CR.utility_inputs(rng, kind, m, L)
    oc = B.OutputConstraints(*CR.draw_constraints(rng, CR.train_mean(la), Kc, eta))
    rows = np.arange(n) % L
    u0 = rng.uniform(-3.0, -1.0, size=L)
    return la, Xc, Z, thetas, params, oc, rows, u0


# ---- the restatement ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", UTILS)
def test_vacuous_constraints_give_the_oracles_plain_monte_carlo_expected_utility(kind):
    la, Xc, Z, thetas, params, oc, rows, u0 = _small(kind)
    mean, var = CE.posterior_noiseless(la, Xc)
    r = CE.constrained_eu_hyper([mean], [var], Z, thetas, rows, u0, kind, params, oc.A, np.full(oc.K, 1e30), oc.eta, n_hyps=3)
    want = 3.0 * CE.plain_mc_eu(mean, var, Z, thetas, rows, kind, params)
    np.testing.assert_allclose(r["G"], want, rtol=1e-12, atol=0)
    np.testing.assert_array_equal(r["P"], np.ones(len(Xc)))


@pytest.mark.parametrize("kind", UTILS)
def test_indicator_limit(kind):
    # the first problem (seeds from 3) with no sample within 50 eta of a constraint boundary: s is 0 or 1 to below 1e-21 there
    for seed in range(3, 40):
        la, Xc, Z, thetas, params, oc, rows, u0 = _small(kind, seed=seed)
        mean, var = CE.posterior_noiseless(la, Xc)
        sg = np.sqrt(var)
        cmin = min(np.min(np.abs(CR.constraint_values(oc.A, oc.b, mean[:, None, :] + sg[:, None, :] * Z[l].T[:, :, None]))) for l in range(len(Z)))
        if cmin > 50e-6:
            break
    assert cmin > 50e-6
    eta = np.full(oc.K, 1e-6)
    a = (Z, thetas, rows, u0, kind, params, oc.A, oc.b, eta)
    soft, hard = CE.constrained_eu(mean, var, *a), CE.constrained_eu(mean, var, *a, hard=True)
    assert 0 < hard["phi_sum"].sum() < Z.shape[1] * len(Xc)                       # some samples feasible, some not
    np.testing.assert_allclose(soft["G"], hard["G"], rtol=1e-12, atol=0)
    np.testing.assert_allclose(soft["phi_sum"], hard["phi_sum"], rtol=1e-12, atol=0)


def test_affine_in_the_infeasible_utility_with_slope_sum_of_one_minus_phi():
    la, Xc, Z, thetas, params, oc, rows, u0 = _small("neg_sq_dist")
    mean, var = CE.posterior_noiseless(la, Xc)
    S = Z.shape[1]

    def G(u):
        return CE.constrained_eu(mean, var, Z, thetas, rows, u, "neg_sq_dist", params, oc.A, oc.b, oc.eta)
    a, b, c = G(u0), G(u0 - 2.0), G(u0 + 0.7)
    slope = S - a["phi_sum"]
    assert slope.min() > 1e-3                                                      # (the constraints bind: there is a slope to see)
    np.testing.assert_allclose(b["G"] - a["G"], -2.0 * slope, rtol=1e-11, atol=1e-12)
    np.testing.assert_allclose(c["G"] - a["G"], 0.7 * slope, rtol=1e-11, atol=1e-12)
    np.testing.assert_array_equal(a["phi_sum"], b["phi_sum"])                      # P does not read u0


@pytest.mark.parametrize("kind", UTILS)
def test_gradient_against_central_differences(kind):
    la, Xc, Z, thetas, params, oc, rows, u0 = _small(kind, n=6)
    a = (Z, thetas, rows, u0, kind, params, oc.A, oc.b, oc.eta)

    def value(X):
        mean, var = CE.posterior_noiseless(la, X)
        return CE.constrained_eu_hyper([mean], [var], *a, n_hyps=2)["G"]
    mean, var, dmean, dvar = CE.posterior_noiseless(la, Xc, grad=True)
    r = CE.constrained_eu_hyper([mean], [var], *a, n_hyps=2, dmeans=[dmean], dvars=[dvar])
    h, fd = 1e-6, np.zeros(Xc.shape)
    for q in range(Xc.shape[1]):
        e = np.zeros(Xc.shape[1])
        e[q] = h
        fd[:, q] = (value(Xc + e) - value(Xc - e)) / (2 * h)
    assert np.abs(r["dG"]).max() > 1e-2
    np.testing.assert_allclose(r["dG"], fd, rtol=1e-5, atol=1e-6 * max(1.0, np.abs(fd).max()))


# ---- the decision property, on the CPU ------------------------------------------------------------------------------------------------
class _ModelStub(object):
    def __init__(self, m, n_samples=1):
        self.output_dim, self._n = m, n_samples

    def number_of_hyps_samples(self):
        return self._n


def _space(d):
    return B.Design_space([{'name': 'x', 'type': 'continuous', 'domain': (0.0, 1.0), 'dimensionality': d}])


def _oracle(m=2, d=2, N=14, seed=3):
    rng = np.random.RandomState(seed)
    X = rng.uniform(size=(N, d))
    Y = [np.sin(3 * X[:, :1] + j) + 0.3 * X[:, 1:2] * (j + 1) for j in range(m)]
    ref = O.MultiOutputGPRef("rbf", [1.0 + 0.2 * j for j in range(m)], [np.full(d, 0.35 + 0.05 * j) for j in range(m)], [1e-6] * m)
    ref.updateModel(X, Y)
    return ref


def test_the_constrained_recommendation_is_feasible_where_the_unconstrained_one_is_not():
    m, d = 2, 2
    ref = _oracle(m, d)
    theta = np.array([[1.10, 0.95]])
    U = B.Utility(parameter_dist=B.ParameterDistribution(support=theta, prob_dist=np.ones(1)), device="neg_sq_dist")
    oc = B.OutputConstraints([[1.0, 0.0]], [0.9], eta=0.02)                        # y_0 <= 0.9 cuts off the outcome the utility aims at
    factory = CE.restated_factory(ref, "neg_sq_dist", 1)
    kw = dict(n_hyps=1, n_starting=40, n_anchor=4, evaluator=factory)
    # the restatement alone first: the plain expected utility peaks at an infeasible posterior mean, the constrained one at a feasible one
    grid = np.stack(np.meshgrid(np.linspace(0, 1, 21), np.linspace(0, 1, 21)), -1).reshape(-1, d)
    Zg = np.random.RandomState(0).normal(size=(1, REC.N_Z_SAMPLES, m))
    rows = np.zeros(len(grid), dtype=int)
    mean_g = ref.predict_noiseless(grid)[0]
    plain = factory(theta, Zg)(grid, rows)[0]
    cons = factory(theta, Zg, oc, np.array([-10.0]))
    assert not oc.feasible(mean_g[:, np.argmax(plain)])
    best = np.argmax(cons(grid, rows)[0])
    assert oc.feasible(mean_g[:, best]) and cons.pof(grid[best:best + 1], [0])[0] >= 0.9
    # ... then the recommendation step
    np.random.seed(5)
    x_free, _ = B.current_marginal_argmaxes(_ModelStub(m), _space(d), U, theta, **kw)
    np.random.seed(5)
    info = {}
    x_con, v_con = B.current_marginal_argmaxes(_ModelStub(m), _space(d), U, theta, constraints=oc, infeasible_utility=-10.0, info=info, **kw)
    assert not oc.feasible(ref.predict_noiseless(x_free)[0][:, 0])
    assert oc.feasible(ref.predict_noiseless(x_con)[0][:, 0])
    assert info["pof"].shape == (1,) and info["pof"][0] >= 0.9
    np.testing.assert_array_equal(info["u_infeasible"], [-10.0])
    assert np.isfinite(v_con[0])


# ---- surface ---------------------------------------------------------------------------------------------------------------------
def test_header_declares_and_library_exports_the_entry_points():
    header = open(os.path.join(ROOT, "include", "bocf_hip.h")).read()
    lib = _ffi.load()
    for name in ENTRY_POINTS:
        assert re.search(r"\bint %s\(bocf_ctx\* ctx" % name, header), name
        assert name in _ffi.SIGNATURES
        assert isinstance(getattr(lib, name), ctypes._CFuncPtr)
    from bocf_amd import build
    assert "ceu.hip" in build.SOURCES
    for name in ("train_utility_range", "expected_utility_constrained"):
        assert getattr(B.multi_outputGP, name).__doc__
    assert "constraints" in B.multi_outputGP(2, fixed_hyps=True)._resident.__slots__ and len(B.multi_outputGP(2)._resident.__slots__) == 10


def test_null_context_refusals_name_the_entry_point():
    lib, dp = _ffi.load(), _ffi.dptr
    th, out = np.zeros((1, 3)), np.empty(1)
    rows = np.zeros(1, dtype=np.int32)

    def bad(rc, name, text):
        msg = lib.bocf_last_error()
        assert rc < 0 and name.encode() in msg and text.encode() in msg, (rc, msg, text)
    bad(lib.bocf_train_utility_range(None, 1, None, 0, dp(th), 3, 1, dp(out), dp(out)), "bocf_train_utility_range", "model not fitted")
    bad(lib.bocf_expected_utility_constrained(None, 1, None, 0, dp(th), 3, 1, dp(out), rows.ctypes.data_as(ctypes.POINTER(ctypes.c_int)), 1, dp(out),
                                              None, None), "bocf_expected_utility_constrained", "model not fitted")


def test_cbo_and_the_recommendation_step_accept_the_new_keywords():
    for f in (B.current_marginal_argmaxes, B.CBO.__init__):
        p = inspect.signature(f).parameters
        assert p["constraints"].default is None and p["infeasible_utility"].default is None
    oc = B.OutputConstraints([[1.0, 0.0]], [0.5])
    U = B.Utility(parameter_dist=B.ParameterDistribution(support=np.array([[0.2, 0.1]]), prob_dist=np.ones(1)), device="neg_sq_dist")

    class Acq(object):
        utility = U

    class Objective(object):
        def evaluate(self, X):
            return [np.full((len(X), 1), 0.8), np.full((len(X), 1), 0.1)], 0.0
    X0 = np.zeros((2, 2))
    bo = B.CBO(_ModelStub(2), _space(2), Objective(), Acq(), None, X0, constraints=oc, infeasible_utility=-7.0)
    assert bo.constraints is oc and bo._constraint_arguments() == {"constraints": oc, "infeasible_utility": -7.0}
    assert bo._marginal_value(np.array([0.2, 0.1]), X0[0], -7.0) == -7.0           # the true outputs (0.8, 0.1) violate y_0 <= 0.5
    plain = B.CBO(_ModelStub(2), _space(2), Objective(), Acq(), None, X0)
    assert plain.constraints is None and plain._constraint_arguments() == {}       # opt-in: nothing passed on
    np.testing.assert_allclose(plain._marginal_value(np.array([0.2, 0.1]), X0[0]), -0.36)
    with pytest.raises(ValueError):
        B.CBO(_ModelStub(2), _space(2), Objective(), Acq(), None, X0, infeasible_utility=-7.0)
    with pytest.raises(ValueError):
        B.current_marginal_argmaxes(_ModelStub(2), _space(2), U, np.array([[0.2, 0.1]]), infeasible_utility=-7.0)
    # a utility without a compiled-in device kind: no host loop on this path
    odd = B.Utility(func=lambda t, y: -np.sum(np.abs(np.asarray(y).T - t).T ** 1.5, axis=0), dfunc=lambda t, y: y,
                    parameter_dist=B.ParameterDistribution(support=np.array([[0.2, 0.1]]), prob_dist=np.ones(1)))
    with pytest.raises(NotImplementedError):
        REC.constrained_device_evaluator(_ModelStub(2), odd, np.array([[0.2, 0.1]]), None, np.zeros(1))


def _quadratic(parameters, Z, constraints=None, u0=None):
    def ev(X, rows, grad=False):
        diff = X - (0.25 + 0.5 * np.tanh(np.asarray(parameters)[rows, :1]))
        return -np.sum(diff ** 2, 1), (-2.0 * diff if grad else None)
    return ev


@pytest.mark.parametrize("branch", ["mean", "closed", "mc"])
def test_rng_order_with_and_without_constraints(branch):
    """Without constraints the draws are the reference's (Z in the Monte-Carlo branch only); with them Z is drawn in every branch, in the
    Monte-Carlo branch's order: per parameter Z (50, m), then one uniform per input dimension."""
    m, d, L, P = 2, 3, 3, 20
    support = np.random.RandomState(5).uniform(-1, 1, size=(L, m))
    dist = B.ParameterDistribution(support=support, prob_dist=np.full(L, 1.0 / L))
    U = B.Utility(func=lambda t, y: np.dot(t, y), parameter_dist=dist, linear=True) if branch == "mean" else B.Utility(parameter_dist=dist, device="neg_sq_dist")
    psi = B.ExpectationUtility(lambda t, mu, var: REC.closed_form("neg_sq_dist", t, mu, var)[0],
                               lambda t, mu, var: REC.closed_form("neg_sq_dist", t, mu, var)[1]) if branch == "closed" else None
    oc = B.OutputConstraints([[1.0, 0.0]], [0.5])

    def restated(with_Z):
        np.random.seed(11)
        Zs, designs = [], []
        for _ in range(L):
            if with_Z:
                Zs.append(np.random.normal(size=(50, m)))
            designs.append(np.stack([np.random.uniform(low=0.0, high=1.0, size=P) for _ in range(d)], 1))
        return Zs, np.stack(designs), np.random.uniform()
    for constrained in (False, True):
        Zs, designs, nxt = restated(constrained or branch == "mc")
        np.random.seed(11)
        info = {}
        kw = dict(constraints=oc, infeasible_utility=-1.0) if constrained else {}
        B.current_marginal_argmaxes(_ModelStub(m), _space(d), U, support, psi, n_starting=P, n_anchor=2, evaluator=_quadratic, info=info, **kw)
        assert np.random.uniform() == nxt
        np.testing.assert_array_equal(info["designs"], designs)
        assert info["branch"] == branch
        if Zs:
            np.testing.assert_array_equal(info["Z"], np.stack(Zs))
        else:
            assert info["Z"] is None
        assert ("u_infeasible" in info) == constrained


def test_an_unconstrained_step_makes_the_calls_it_made_and_a_constrained_one_the_new_ones(monkeypatch):
    """The recorded traces of tests/golden/model_calls.json replay unchanged (the three scenarios hold no OutputConstraints in the
    recommendation step), and a recommendation step on the recording stand-in calls the new entry points only with constraints."""
    for name, scenario in MC.SCENARIOS:
        MC._check(name, scenario, monkeypatch)
    new = {"bocf_train_utility_range", "bocf_expected_utility_constrained", "bocf_set_output_constraints"}
    rng = np.random.RandomState(0)
    X, Y = rng.uniform(size=(8, 2)), [rng.normal(size=(8, 1)) for _ in range(2)]
    support = rng.uniform(size=(2, 2))
    U = B.Utility(parameter_dist=B.ParameterDistribution(support=support, prob_dist=np.array([0.5, 0.5])), device="neg_sq_dist")
    oc = B.OutputConstraints([[1.0, 0.0]], [0.5])
    traces = []
    for kw in ({}, dict(constraints=None), dict(constraints=oc)):
        lib = MC.RecordingLibrary()
        monkeypatch.setattr(_ffi, "load", lambda lib=lib: lib)
        model = B.multi_outputGP(2, fixed_hyps=True, noise_var=[1e-4] * 2)
        model.updateModel(X, Y)
        np.random.seed(2)
        with np.errstate(all="ignore"):
            try:
                B.current_marginal_argmaxes(model, _space(2), U, support, n_starting=6, n_anchor=2, **kw)
            except Exception:                                                      # (the stand-in leaves outputs uninitialised: the optimiser may give up)
                pass
        traces.append([c[0] for c in lib.calls if c[0] != "#"])
    assert traces[0] and traces[0][:8] == traces[1][:8] and not new & set(traces[0]) and not new & set(traces[1])
    assert "bocf_expected_utility" in traces[0]
    con = traces[2]
    assert "bocf_expected_utility" not in con
    first = [con.index(n) for n in ("bocf_set_output_constraints", "bocf_train_utility_range", "bocf_set_eu_samples", "bocf_expected_utility_constrained")]
    assert first == sorted(first)
    assert con.count("bocf_set_output_constraints") == 1 and con.count("bocf_set_eu_samples") == 1


# ---- the argument checks of the two entry points, through the stand-alone driver ---------------------------------------------------------
NO_PROGRAM = "the constrained expected utility does not take a utility program (BOCF_UTIL_PROGRAM): use one of the compiled-in utilities"
CHECKS = ["model not fitted", NO_PROGRAM, "no output constraints resident", "not a whole number of hyper-samples", "more outputs per hyper-sample",
          "given for another m", "best_group", "L out of range", "no Monte-Carlo samples set (bocf_set_eu_samples)", "fewer Monte-Carlo sample blocks",
          "another output count", "u_infeasible is null", "u_infeasible has a non-finite entry", "n_hyps must be >= 1", "n_hyps exceeds",
          "host-given posterior", "input dimension too large", "null output / row_param", "row_param out of range"]


@pytest.fixture(scope="module", params=["plain", "sanitized"])
def driver(request, tmp_path_factory):
    if not os.path.exists(CLANG):
        pytest.skip("no clang++ next to hipcc")
    exe = str(tmp_path_factory.mktemp("ceu_args") / ("ceu_args_driver_" + request.param))
    extra = ["-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-g"] if request.param == "sanitized" else []
    subprocess.check_call([CLANG, "-std=c++17", "-O2", "-Wall", "-Werror"] + extra + [os.path.join(ROOT, "tests", "ceu_args_driver.cpp"), "-o", exe])
    return exe


def _line(who, need=1, **kw):
    c = dict(fitted=1, canned=0, m=4, H=1, best_group=-1, cq_K=2, cq_m=4, eu_S=50, eu_L=3, eu_m=4, d=3, C=5,
             kind=1, n_params=0, params_null=1, theta_null=0, theta_dim=4, L=3, u0=1, rows=1, n_hyps=1, val_null=0, grad=0)
    c.update(kw)
    return ("%s|%d %d %d %d %d %d %d %d %d %d %d %d %d|%d %d %d %d %d %d|%d %d %d %d %d"
            % (who, c["fitted"], c["canned"], c["m"], c["H"], c["best_group"], c["cq_K"], c["cq_m"], c["eu_S"], c["eu_L"], c["eu_m"], c["d"], c["C"], need,
               c["kind"], c["n_params"], c["params_null"], c["theta_null"], c["theta_dim"], c["L"], c["u0"], c["rows"], c["n_hyps"], c["val_null"], c["grad"]))


def _verdicts(driver, lines):
    out = subprocess.run([driver], input="".join(l + "\n" for l in lines), capture_output=True, text=True)
    assert out.returncode == 0, out.stderr
    got = out.stdout.split("\n")[:-1]
    assert len(got) == len(lines), (got, out.stderr)
    return got


# one fault per check of bocf_expected_utility_constrained, in the order the entry point makes them
FAULTS = [dict(fitted=0), dict(kind=5), dict(cq_K=0), dict(m=5, H=2), dict(m=17, cq_m=17, eu_m=17, theta_dim=16, kind=2), dict(cq_m=3), dict(best_group=1),
          dict(L=0), dict(eu_S=0), dict(eu_L=2), dict(eu_m=3), dict(u0=0), dict(u0=2), dict(n_hyps=0), dict(m=8, H=2, n_hyps=3), dict(canned=1, grad=1),
          dict(d=65, grad=1), dict(val_null=1), dict(rows=2)]


def test_each_refusal_names_the_entry_point_in_its_own_words(driver):
    who = "bocf_expected_utility_constrained"
    assert len(FAULTS) == len(CHECKS)
    got = _verdicts(driver, [_line(who, **f) for f in FAULTS] + [_line(who), _line(who, C=0, rows=0, val_null=1), _line(who, u0=3), _line(who, rows=3),
                                                                    _line(who, rows=0), _line(who, kind=7), _line(who, canned=1), _line(who, d=65),
                                                                    _line(who, m=8, H=2, n_hyps=2), _line(who, n_hyps=12)])
    for g, text, f in zip(got, CHECKS, FAULTS):
        assert g.startswith(who + ": ") and text in g, (f, g)
    assert got[len(FAULTS):] == ["ok 4", "nothing 4", who + ": u_infeasible has a non-finite entry", who + ": row_param out of range [0, L)",
                                 who + ": null output / row_param", who + ": unknown utility kind", "ok 4", "ok 4", "ok 4", "ok 4"]


def test_the_earlier_of_two_faults_is_reported(driver):
    who = "bocf_expected_utility_constrained"
    pairs = []
    for i in range(len(FAULTS) - 1):
        a, b = FAULTS[i], FAULTS[i + 1]
        if set(a) & set(b) or i in (3, 4, 14):                                      # (the layout cases set m, H together: they meet their neighbours below)
            continue
        pairs.append((dict(a, **b), CHECKS[i]))
    pairs += [(dict(m=5, H=2, cq_m=3), CHECKS[3]), (dict(m=17, cq_m=3, eu_m=17, theta_dim=16, kind=2), CHECKS[4]), (dict(cq_m=3, best_group=1), CHECKS[5]),
              (dict(eu_S=0, eu_L=2), CHECKS[8]), (dict(eu_L=2, eu_m=3), CHECKS[9]), (dict(u0=2, n_hyps=0), CHECKS[12]),
              (dict(m=8, H=2, n_hyps=3, canned=1, grad=1), CHECKS[14]), (dict(canned=1, grad=1, d=65), CHECKS[15]), (dict(val_null=1, rows=2), CHECKS[17]),
              (dict(fitted=0, kind=5, cq_K=0), CHECKS[0]), (dict(kind=5, L=0), CHECKS[1]), (dict(cq_K=0, L=0, theta_null=1), CHECKS[2])]
    assert len(pairs) >= 20
    for (f, text), g in zip(pairs, _verdicts(driver, [_line(who, **f) for f, _ in pairs])):
        assert g.startswith(who + ": ") and text in g, (f, g, text)


def test_the_utility_range_reads_no_constraint_and_no_samples(driver):
    who = "bocf_train_utility_range"
    got = _verdicts(driver, [_line(who, need=0, cq_K=0, cq_m=0, eu_S=0, u0=0, rows=0, val_null=1), _line(who, need=0, fitted=0), _line(who, need=0, kind=5),
                             _line(who, need=0, theta_dim=3), _line(who, need=0, kind=4, m=3, theta_dim=1), _line(who, need=0, kind=3, n_params=2, params_null=0),
                             _line(who, need=0, m=8, H=2, best_group=2), _line(who, need=0, m=8, H=2, best_group=1)])
    assert got == ["ok 4", who + ": model not fitted", who + ": " + NO_PROGRAM, who + ": theta_dim must equal m", who + ": rosenbrock utility needs even m",
                   who + ": neg_exp_cos needs m weights", who + ": option best_group is not a valid hyper-sample index", "ok 4"]
