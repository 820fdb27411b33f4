"""Quantile / tail-mean acquisitions and the closed-form confidence bound, CPU side: the NumPy restatement (tests/risk_ref.py) against
itself -- np.partition, the tail-mean identities, its pathwise gradient against central differences of its own value --, the public
surface, the rank the Python classes hand to the device, and the refusals of the C ABI that need no GPU."""
import ctypes
import os
import re
import subprocess
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import constrained_ref as CR  # noqa: E402
import kg_ref as K  # noqa: E402
import risk_ref as RR  # noqa: E402

import bocf_amd as B  # noqa: E402
from bocf_amd import _ffi  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENTRY_POINTS = ["bocf_acq_risk", "bocf_acq_linear_ucb"]
UTILS = ["linear", "neg_sq_dist", "neg_sum_exp", "neg_exp_cos", "rosenbrock"]
KINDS = [RR.QUANTILE, RR.UPPER_TAIL, RR.LOWER_TAIL]


# ---- the restatement ------------------------------------------------------------------------------------------------------------
def test_quantile_agrees_with_np_partition_and_ties_go_by_index():
    rng = np.random.RandomState(0)
    for S in (1, 2, 7, 64, 65, 200):
        for u in (rng.normal(size=S), np.round(rng.normal(size=S), 1), np.zeros(S), np.where(rng.uniform(size=S) < 0.2, np.nan, rng.normal(size=S))):
            clean = np.where(np.isnan(u), -np.inf, u)
            for k in sorted({0, S // 2, S - 1}):
                rho, T, gap = RR.statistic(u, RR.QUANTILE, k)
                assert rho == np.partition(clean, k)[k] and clean[T[0]] == rho and gap >= 0
                # exactly k samples before it in (value, index) order
                before = np.sum((clean < rho) | ((clean == rho) & (np.arange(S) < T[0])))
                assert before == k
                up, Tu, _ = RR.statistic(u, RR.UPPER_TAIL, k)
                lo, Tl, _ = RR.statistic(u, RR.LOWER_TAIL, k)
                assert len(Tu) == S - k and len(Tl) == k + 1 and set(Tu) & set(Tl) == {T[0]} and len(set(Tu) | set(Tl)) == S
                if np.all(np.isfinite(clean)):
                    np.testing.assert_allclose(up, np.sort(clean)[k:].mean(), rtol=1e-13, atol=1e-300)
                    np.testing.assert_allclose(lo, np.sort(clean)[:k + 1].mean(), rtol=1e-13, atol=1e-300)
    # a tie across rank k: the lower index comes first; -0.0 and +0.0 tie as numbers
    u = np.array([1.0, 0.0, 1.0, -0.0, 1.0])
    assert [RR.statistic(u, RR.QUANTILE, k)[1][0] for k in range(5)] == [1, 3, 0, 2, 4]
    assert RR.statistic(np.array([np.nan, -np.inf, 0.0]), RR.QUANTILE, 0)[1][0] == 0          # NaN ranks as -inf, by index
    assert RR.statistic(np.array([np.nan, 1.0]), RR.LOWER_TAIL, 1)[0] == -np.inf                 # ... and counts as -inf


def test_tail_means_at_the_ends_are_the_plain_mean():
    rng = np.random.RandomState(1)
    m, n, S = 3, 9, 40
    mean, var, W = rng.uniform(-1, 1, size=(m, n)), rng.uniform(0.01, 0.5, size=(m, n)), rng.normal(size=(S, m))
    thetas, prob = rng.uniform(-0.5, 0.5, size=(2, m)), np.array([0.3, 0.7])
    y = mean[:, None, :] + np.sqrt(var)[:, None, :] * W.T[:, :, None]
    from oracle import cpu_ref as R
    plain = sum(p * R.utility_eval("neg_sq_dist", th, y.reshape(m, -1)).reshape(S, n).mean(0) for p, th in zip(prob, thetas))
    up = RR.risk(mean, var, W, thetas, prob, "neg_sq_dist", None, RR.UPPER_TAIL, 0)["alpha"]
    lo = RR.risk(mean, var, W, thetas, prob, "neg_sq_dist", None, RR.LOWER_TAIL, S - 1)["alpha"]
    np.testing.assert_allclose(up, plain, rtol=1e-13)
    np.testing.assert_allclose(lo, plain, rtol=1e-13)
    # the two ends of the quantile are the extremes, and the tails there are the quantile itself
    q0 = RR.risk(mean, var, W, thetas, prob, "neg_sq_dist", None, RR.QUANTILE, 0)["alpha"]
    q1 = RR.risk(mean, var, W, thetas, prob, "neg_sq_dist", None, RR.QUANTILE, S - 1)["alpha"]
    np.testing.assert_array_equal(RR.risk(mean, var, W, thetas, prob, "neg_sq_dist", None, RR.LOWER_TAIL, 0)["alpha"], q0)
    np.testing.assert_array_equal(RR.risk(mean, var, W, thetas, prob, "neg_sq_dist", None, RR.UPPER_TAIL, S - 1)["alpha"], q1)
    assert np.all(q0 <= lo) and np.all(up <= q1)


def _small(util, seed=3, N=14, d=2, m=2, S=40, L=2, n=12):
    kinds = ["se", "matern52", "rbf", "matern32"][:m]
    X, Y, var, ls, nz, Xc = K.problem(kinds, N, d, n, seed, noise=1e-4)
    la = K.LookAhead.fit(kinds, X, Y, var, ls, nz)
    rng = np.random.RandomState(100 + seed)
    W = rng.normal(size=(S, m))
    thetas, params = CR.utility_inputs(rng, util, m, L)
    return la, Xc, W, thetas, rng.dirichlet(np.ones(L)), params


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("util", UTILS)
def test_gradient_against_central_differences(util, kind):
    """The restatement's pathwise gradient against central differences of its own value (rtol 1e-3, atol 1e-6 max(1, |g|max), the
    finite-difference gate of the other restatements) on the candidates whose u_(k) is separated from its neighbours by more than 1e-3 of the
    largest sample: the selected set is then the same at x - h, x and x + h."""
    la, Xc, W, thetas, prob, params = _small(util, seed=5)
    S, k = W.shape[0], 29
    post = CR.posterior(la, Xc, grad=True)
    r = RR.risk(post[0], post[1], W, thetas, prob, util, params, kind, k, post[2], post[3])
    keep = r["gap"].min(1) > 1e-3 * r["scale"]
    assert keep.sum() >= 4
    h, fd = 1e-6, np.zeros_like(Xc)
    for q in range(Xc.shape[1]):
        Xp, Xm = Xc.copy(), Xc.copy()
        Xp[:, q] += h
        Xm[:, q] -= h
        fd[:, q] = (RR.risk(*CR.posterior(la, Xp), W, thetas, prob, util, params, kind, k)["alpha"]
                    - RR.risk(*CR.posterior(la, Xm), W, thetas, prob, util, params, kind, k)["alpha"]) / (2 * h)
    g = r["dalpha"]
    print("%s kind %d: gradient vs central differences on %d of %d candidates: max abs difference %.3g, gradient scale %.3g"
          % (util, kind, keep.sum(), len(Xc), np.abs(g[keep] - fd[keep]).max(), np.abs(g).max()))
    assert np.abs(g[keep]).max() > 0
    np.testing.assert_allclose(g[keep], fd[keep], rtol=1e-3, atol=1e-6 * max(1.0, np.abs(g).max()))


def test_linear_ucb_restatement():
    la, Xc, W, thetas, prob, params = _small("linear", seed=6)
    post = CR.posterior(la, Xc, grad=True)
    v0 = RR.linear_ucb(post[0], post[1], thetas, prob, 0.0)
    np.testing.assert_allclose(v0, prob.dot(thetas.dot(post[0])), rtol=1e-14)
    v, g = RR.linear_ucb(post[0], post[1], thetas, prob, 2.0, post[2], post[3])
    assert np.all(v > v0)
    h, fd = 1e-6, np.zeros_like(Xc)
    for q in range(Xc.shape[1]):
        Xp, Xm = Xc.copy(), Xc.copy()
        Xp[:, q] += h
        Xm[:, q] -= h
        fd[:, q] = (RR.linear_ucb(*CR.posterior(la, Xp), thetas, prob, 2.0) - RR.linear_ucb(*CR.posterior(la, Xm), thetas, prob, 2.0)) / (2 * h)
    np.testing.assert_allclose(g, fd, rtol=1e-3, atol=1e-6 * max(1.0, np.abs(g).max()))
    # with one theta the bound at the level's normal quantile is the quantile of the (Gaussian) linear utility: uUCB's large-S limit
    rng = np.random.RandomState(2)
    Wbig = rng.normal(size=(4000, 2))
    q = RR.risk(post[0], post[1], Wbig, thetas[:1], None, "linear", None, RR.QUANTILE, RR.rank_of(0.9, 4000))["alpha"]
    np.testing.assert_allclose(q, RR.linear_ucb(post[0], post[1], thetas[:1], None, 1.2815515655446004), atol=0.1 * np.sqrt(post[1].max()))


# ---- surface ---------------------------------------------------------------------------------------------------------------------
def test_header_declares_and_library_exports_the_entry_points():
    header = open(os.path.join(ROOT, "include", "bocf_hip.h")).read()
    lib = _ffi.load()
    for name in ENTRY_POINTS:
        assert re.search(r"\bint %s\(bocf_ctx\* ctx" % name, header), name
        assert name in _ffi.SIGNATURES
        assert isinstance(getattr(lib, name), ctypes._CFuncPtr)
    for name, value in (("BOCF_RISK_QUANTILE", _ffi.RISK_QUANTILE), ("BOCF_RISK_UPPER_TAIL", _ffi.RISK_UPPER_TAIL), ("BOCF_RISK_LOWER_TAIL", _ffi.RISK_LOWER_TAIL)):
        assert re.search(r"\b%s = %d\b" % (name, value), header), name
    assert re.search(r"#define BOCF_RISK_MAX_SAMPLES %d\b" % _ffi.RISK_MAX_SAMPLES, header)
    assert (RR.QUANTILE, RR.UPPER_TAIL, RR.LOWER_TAIL) == (_ffi.RISK_QUANTILE, _ffi.RISK_UPPER_TAIL, _ffi.RISK_LOWER_TAIL)
    from bocf_amd import build
    assert "risk.hip" in build.SOURCES and "capi_risk.hip" in build.SOURCES


def test_abi_refusals_that_need_no_gpu():
    lib, dp = _ffi.load(), _ffi.dptr
    th = np.zeros((1, 3))

    def bad(rc, name, text):
        msg = lib.bocf_last_error()
        assert rc < 0 and name.encode() in msg and text.encode() in msg, (rc, msg, text)

    def risk(kind=_ffi.RISK_QUANTILE, rank=0, util=_ffi.UTIL_NEG_SQ_DIST):
        return lib.bocf_acq_risk(None, kind, rank, util, None, 0, dp(th), 3, None, 1, None, None)
    who = "bocf_acq_risk"
    bad(risk(kind=3), who, "unknown risk kind")
    bad(risk(kind=-1), who, "unknown risk kind")
    bad(risk(rank=-1), who, "rank out of range")
    bad(risk(util=_ffi.UTIL_PROGRAM), who, "BOCF_UTIL_PROGRAM")
    bad(risk(util=7), who, "unknown utility kind")
    bad(risk(), who, "model not fitted")
    who = "bocf_acq_linear_ucb"
    for kappa in (np.inf, -np.inf, np.nan):
        bad(lib.bocf_acq_linear_ucb(None, kappa, dp(th), None, 1, None, None), who, "kappa must be finite")
    bad(lib.bocf_acq_linear_ucb(None, 2.0, dp(th), None, 1, None, None), who, "model not fitted")


# ---- every argument check of the two entry points, through the stand-alone driver (bocf_amd/csrc/risk_args.h) -----------------------------
# A fit takes d <= 32 today, so no fitted context reaches the d > 64 refusal of the gradient forms: it is driven here, where the record of
# the context is the test's to write.
CLANG = "/opt/rocm/lib/llvm/bin/clang++"
CHECKS = ["unknown risk kind", "rank out of range", "BOCF_UTIL_PROGRAM", "unknown utility kind", "model not fitted", "not a whole number of hyper-samples",
          "more outputs per hyper-sample", "L out of range", "theta must be", "theta_dim must equal m", "rosenbrock utility needs even m",
          "no Monte-Carlo samples set (bocf_set_mc_samples)", "S <= 4096", "rank out of range", "no resident candidates", "host-given posterior",
          "input dimension too large (gradients: d <= 64)"]
# one fault per check of bocf_acq_risk, in the order the entry point makes them
FAULTS = [dict(risk_kind=3), dict(rank=-1), dict(kind=5), dict(kind=7), dict(fitted=0), dict(m=5, H=2), dict(m=17, theta_dim=16, kind=2), dict(L=0),
          dict(theta_null=1), dict(theta_dim=3), dict(kind=4, theta_dim=1, m=3), dict(S_mc=0), dict(S_mc=4097), dict(rank=25), dict(C=0),
          dict(canned=1, grad=1), dict(d=65, grad=1)]


@pytest.fixture(scope="module", params=["plain", "sanitized"])
def driver(request, tmp_path_factory):
    assert os.path.exists(CLANG), "no clang++ next to hipcc"
    exe = str(tmp_path_factory.mktemp("risk_args") / ("risk_args_driver_" + request.param))
    extra = ["-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-g"] if request.param == "sanitized" else []
    subprocess.check_call([CLANG, "-std=c++17", "-O2", "-Wall", "-Werror"] + extra + [os.path.join(ROOT, "tests", "risk_args_driver.cpp"), "-o", exe])
    return exe


def _line(who, kappa="none", **kw):
    c = dict(fitted=1, canned=0, m=4, H=1, S_mc=25, d=3, C=5, risk_kind=0, rank=22, kind=1, n_params=0, params_null=1, theta_null=0, theta_dim=4, L=3, grad=0)
    c.update(kw)
    return ("%s|%d %d %d %d %d %d %d|%d %d %d %d %d %d %d %d %d|%s"
            % (who, c["fitted"], c["canned"], c["m"], c["H"], c["S_mc"], c["d"], c["C"], c["risk_kind"], c["rank"], c["kind"], c["n_params"],
               c["params_null"], c["theta_null"], c["theta_dim"], c["L"], c["grad"], kappa))


def _verdicts(driver, lines):
    out = subprocess.run([driver], input="".join(l + "\n" for l in lines), capture_output=True, text=True)
    assert out.returncode == 0, out.stderr
    got = out.stdout.split("\n")[:-1]
    assert len(got) == len(lines), (got, out.stderr)
    return got


def test_each_refusal_names_the_entry_point_in_its_own_words(driver):
    who = "bocf_acq_risk"
    assert len(FAULTS) == len(CHECKS)
    for g, text, f in zip(_verdicts(driver, [_line(who, **f) for f in FAULTS]), CHECKS, FAULTS):
        assert g.startswith(who + ": ") and text in g, (f, g)
    # what is accepted: the ends of every range, the value form on a host-given posterior and at any d, the gradient form at d = 64
    ok = [_line(who), _line(who, rank=0), _line(who, rank=24), _line(who, risk_kind=2, S_mc=4096, rank=4095), _line(who, canned=1), _line(who, d=65),
          _line(who, d=64, grad=1), _line(who, m=8, H=2), _line(who, m=16, theta_dim=16), _line(who, L=32), _line(who, kind=4, theta_dim=1)]
    assert _verdicts(driver, ok) == ["ok 4"] * 7 + ["ok 4", "ok 16", "ok 4", "ok 4"]
    # the closed form: theta is (L, m), so there is no theta_dim to get wrong
    who = "bocf_acq_linear_ucb"
    bad = [(_line(who, "inf"), "kappa must be finite"), (_line(who, "-inf"), "kappa must be finite"), (_line(who, "nan"), "kappa must be finite"),
           (_line(who, "2", fitted=0), "model not fitted"), (_line(who, "2", m=5, H=2), "whole number of hyper-samples"),
           (_line(who, "2", m=17), "more outputs per hyper-sample"), (_line(who, "2", L=0), "L out of range"), (_line(who, "2", L=33), "L out of range"),
           (_line(who, "2", theta_null=1), "theta must be"), (_line(who, "2", C=0), "no resident candidates"),
           (_line(who, "2", canned=1, grad=1), "host-given posterior"), (_line(who, "2", d=65, grad=1), "input dimension too large (gradients: d <= 64)")]
    for (_, text), g in zip(bad, _verdicts(driver, [l for l, _ in bad])):
        assert g.startswith(who + ": ") and text in g, (text, g)
    ok = [_line(who, "2"), _line(who, "0"), _line(who, "-1.5"), _line(who, "2", S_mc=0), _line(who, "2", canned=1), _line(who, "2", d=65), _line(who, "2", d=64, grad=1)]
    assert _verdicts(driver, ok) == ["ok 4"] * 7


def test_the_earlier_of_two_faults_is_reported(driver):
    who = "bocf_acq_risk"
    pairs = [(dict(risk_kind=9, rank=-1), CHECKS[0]), (dict(rank=-1, kind=5), CHECKS[1]), (dict(kind=5, fitted=0), CHECKS[2]), (dict(fitted=0, L=0), CHECKS[4]),
             (dict(L=0, S_mc=0), CHECKS[7]), (dict(S_mc=0, C=0), CHECKS[11]), (dict(rank=30, C=0), CHECKS[13]), (dict(C=0, d=65, grad=1), CHECKS[14]),
             (dict(canned=1, d=65, grad=1), CHECKS[15])]
    for (f, text), g in zip(pairs, _verdicts(driver, [_line(who, **f) for f, _ in pairs])):
        assert text in g, (f, g)


@pytest.mark.parametrize("S", [1, 2, 25, 64, 100, 4096])
def test_rank_mapping_of_the_classes(S):
    """k = min(S - 1, floor(level * S)), in double precision, once, in Python."""
    levels = [0.0, 1.0 / S, 0.5, 1.0 - 1.0 / S, 1.0]
    want = [min(S - 1, int(np.floor(lv * S))) for lv in levels]
    assert want[0] == 0 and want[-1] == S - 1 and want[2] == min(S - 1, S // 2) and all(0 <= k < S for k in want)
    U = B.Utility(parameter_dist=B.ParameterDistribution(support=np.array([[0.1, 0.2, 0.3]]), prob_dist=np.array([1.0])), device="neg_sq_dist")
    for lv, k in zip(levels, want):
        assert B.acquisitions.risk_rank(lv, S) == k == RR.rank_of(lv, S)
        for cls, kw in ((B.uUCB, {}), (B.uCVaR, {"tail": "lower"}), (B.uCVaR, {"tail": "upper"})):
            model = _MockModel(3)
            acq = cls(model, None, utility=U, level=lv, **kw)
            acq.W_samples = np.zeros((S, 3))
            acq._compute_acq(np.zeros((2, 2)))
            assert acq.rank == k and model.calls[-1][1] == k
    for lv in (-0.1, 1.1, np.nan):
        with pytest.raises(ValueError):
            B.uUCB(_MockModel(3), None, utility=U, level=lv)


class _MockModel(object):
    analytical_gradient_prediction = True

    def __init__(self, m):
        self.output_dim, self.calls = m, []

    def number_of_hyps_samples(self):
        return 1

    def acq_linear(self, *a, **kw):
        raise AssertionError("not used")

    def acq_risk(self, X, kind, rank, util_kind, util_params, thetas, prob, W=None, n_hyps=None, grad=False, fetch=True):
        self.calls.append(("risk", rank, kind, util_kind, np.array(thetas), None if prob is None else np.array(prob), np.array(W), grad))
        X = np.atleast_2d(X)
        return (X.sum(1), np.ones(X.shape)) if grad else X.sum(1)

    def acq_linear_ucb(self, X, kappa, thetas, prob, n_hyps=None, grad=False, fetch=True):
        self.calls.append(("ucb", kappa, np.array(thetas), None if prob is None else np.array(prob), n_hyps, grad))
        X = np.atleast_2d(X)
        return (X.sum(1), np.ones(X.shape)) if grad else X.sum(1)


class _Parent(object):
    """What uEI_noiseless needs of a device model."""
    analytical_gradient_prediction = True

    def __init__(self, m):
        self.output_dim = m

    def number_of_hyps_samples(self):
        return 1

    def acq_linear(self, *a, **kw):
        raise AssertionError("not used")

    def acq_mc(self, X, kind, util_kind, util_params, thetas, prob, W=None, fetch=True, n_hyps=None, program=None):
        return np.zeros(len(np.atleast_2d(X)))

    def acq_mc_grad(self, X, util_kind, util_params, thetas, prob, W=None, n_hyps=None, program=None):
        X = np.atleast_2d(X)
        return np.zeros(len(X)), np.zeros(X.shape)


def test_exports_class_surface_and_rng_touchpoints():
    for name in ("uUCB", "uCVaR", "maUCB", "UCB"):
        cls = getattr(B, name)
        assert cls is getattr(B.acquisitions, name) and issubclass(cls, B.AcquisitionBase)
        assert cls.analytical_gradient_prediction is True and cls._device_refine is False
    assert issubclass(B.UCB, B.maUCB)
    for name in ("acq_risk", "acq_linear_ucb"):
        assert getattr(B.multi_outputGP, name).__doc__
    support = np.array([[0.2, 0.3, 0.5], [0.6, 0.1, 0.3]])
    X = np.random.RandomState(0).uniform(size=(4, 2))
    # the same np.random draws as uEI_noiseless, in the constructor and per call; update_Z_samples redraws W alone
    out = []
    for cls in (B.uEI_noiseless, B.uUCB, B.uCVaR):
        for full in (True, False):
            dist = B.ParameterDistribution(support=support if full else np.repeat(support, 10, 0), prob_dist=np.array([0.25, 0.75]) if full else None)
            U = B.Utility(parameter_dist=dist, device="neg_sq_dist")
            np.random.seed(11)
            acq = cls(_Parent(3) if cls is B.uEI_noiseless else _MockModel(3), None, utility=U)
            acq._compute_acq(X)
            acq._compute_acq_withGradients(X)
            acq.update_Z_samples(7)
            out.append((acq.W_samples, np.array(acq.utility_params_samples), np.random.uniform()))
    for i in (2, 3, 4, 5):
        np.testing.assert_array_equal(out[i % 2][0], out[i][0])
        np.testing.assert_array_equal(out[i % 2][1], out[i][1])
        assert out[i % 2][2] == out[i][2]
    # what reaches the model
    U = B.Utility(parameter_dist=B.ParameterDistribution(support=support, prob_dist=np.array([0.25, 0.75])), device="neg_sq_dist")
    for cls, kw, kind in ((B.uUCB, {}, _ffi.RISK_QUANTILE), (B.uCVaR, {}, _ffi.RISK_LOWER_TAIL), (B.uCVaR, {"tail": "upper", "level": 0.8}, _ffi.RISK_UPPER_TAIL)):
        model = _MockModel(3)
        acq = cls(model, None, utility=U, **kw)
        assert acq.level == kw.get("level", 0.9 if cls is B.uUCB else 0.1) and acq.analytical_gradient_acq
        v = acq._compute_acq(X)
        assert v.shape == (4, 1) and np.array_equal(v[:, 0], X.sum(1))
        ev = model.calls[-1]
        assert ev[1] == RR.rank_of(acq.level, 25) and ev[2] == kind and ev[3] == _ffi.UTIL_NEG_SQ_DIST and ev[7] is False
        assert np.array_equal(ev[4], support) and np.array_equal(ev[5], [0.25, 0.75]) and np.array_equal(ev[6], acq.W_samples)
        f, df = acq.acquisition_function_withGradients(X)
        assert model.calls[-1][7] is True and np.array_equal(f[:, 0], -X.sum(1)) and np.array_equal(df, -np.ones(X.shape))
        with pytest.raises(NotImplementedError, match="refine='device' does not cover %s" % cls.__name__):
            acq.device_refine_objective()
    with pytest.raises(ValueError):
        B.uCVaR(_MockModel(3), None, utility=U, tail="middle")
    # no host fallback and no utility program; the error names the way out
    dist = B.ParameterDistribution(support=np.array([[0.1, 0.2, 0.3]]), prob_dist=np.array([1.0]))
    odd = B.uUCB(_MockModel(3), None, utility=B.Utility(func=lambda t, y: -np.sum(np.abs(y)), dfunc=lambda t, y: -np.sign(y), parameter_dist=dist))
    for call in (odd._compute_acq, odd._compute_acq_withGradients):
        with pytest.raises(NotImplementedError, match=r"Utility\(\.\.\., device=\.\.\."):
            call(X)
    with pytest.raises(TypeError):
        B.uUCB(_Parent(3), None, utility=U)._compute_acq(X)            # not a device model with the entry point
    # the closed form: a linear utility, maEI's parameter conventions
    lin = B.Utility(parameter_dist=B.ParameterDistribution(support=support, prob_dist=np.array([0.25, 0.75])), linear=True)
    model = _MockModel(3)
    acq = B.maUCB(model, None, utility=lin)
    assert acq.exploration_weight == 2.0
    v, dv = acq._compute_acq_withGradients(X)
    ev = model.calls[-1]
    assert ev[0] == "ucb" and ev[1] == 2.0 and np.array_equal(ev[2], support) and np.array_equal(ev[3], [0.25, 0.75]) and ev[5] is True
    assert np.array_equal(v[:, 0], X.sum(1)) and dv.shape == X.shape
    assert B.UCB(_MockModel(1), None, utility=B.Utility(parameter_dist=B.ParameterDistribution(support=np.array([[1.0]]), prob_dist=np.array([1.0])),
                                                        linear=True), exploration_weight=0.5).n_hyps_samples == 1
    with pytest.raises(NotImplementedError, match="LINEAR"):
        B.maUCB(_MockModel(3), None, utility=U)._compute_acq(X)
    with pytest.raises(ValueError):
        B.maUCB(_MockModel(3), None, utility=lin, exploration_weight=np.inf)
    with pytest.raises(NotImplementedError, match="refine='device' does not cover maUCB"):
        acq.device_refine_objective()
