"""Log-space expected improvement, CPU side: the NumPy restatement (tests/logei_ref.py) against mpmath at 60 digits, against the oracle's
closed-form and Monte-Carlo EI, its gradients against central differences of its own value, the argument checks of the two entry points
through their stand-alone driver, and the Python classes on a stub model.

Gates against mpmath: the errors measured on these points times 4 -- log h 3e-15 relative to max(1, |log h|), log g 1e-12 absolute (the
direct difference 1 - |z| R loses eps z^2, worst just below the switch to the series at |z| = 30), r 1e-12 relative, log psi 1e-15 relative to
max(1, |log psi|).  psi' / psi is assembled as exp of sums of logarithms of magnitude up to 3 log(1e300) = 2100, so it carries that many
roundings: 2100 x 2.2e-16 x 4 = 2e-12 relative."""
import ctypes
import os
import re
import subprocess
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
from oracle import cpu_ref as R  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENTRY_POINTS = ["bocf_acq_log_linear", "bocf_acq_log_mc"]
UTILS = ["linear", "neg_sq_dist", "neg_sum_exp", "neg_exp_cos", "rosenbrock"]
Z_POINTS = [8.0, 1.0, 0.0, -1.0, np.nextafter(-1.0, 0.0), np.nextafter(-1.0, -2.0), -5.0, -29.999, -30.0, -30.001, -38.0, -40.0, -1e3, -1e6, -2.0 ** 26, -1e9,
            -1e12]
DIGITS = 60               # of the mpmath side, set locally around every use (the precision is global state of mpmath)


# ---- the restatement against mpmath ------------------------------------------------------------------------------------------------
def _exact_h(z):
    with mp.workdps(DIGITS):                               # (phi + z Phi cancels to 1 / z^2 of its terms: 24 digits at z = -1e12)
        z = mp.mpf(float(z))
        phi, Phi = mp.exp(-z * z / 2) / mp.sqrt(2 * mp.pi), mp.erfc(-z / mp.sqrt(2)) / 2
        h = phi + z * Phi
        return mp.log(h), Phi / h, mp.log(h / phi)


def test_log_h_and_r_against_mpmath():
    zs = np.array(Z_POINTS + list(-np.logspace(-3, 12, 400)))
    lh, r = LR.log_h(zs)
    e_h = e_r = e_g = 0.0
    for z, a, b in zip(zs, lh, r):
        L, Rr, G = _exact_h(z)
        e_h = max(e_h, float(abs(a - L) / max(1, abs(L))))
        e_r = max(e_r, float(abs(b - Rr) / abs(Rr)))
        if z <= -1.0:
            e_g = max(e_g, float(abs(LR.log_g_and_R(np.array([z]))[0][0] - G)))
    print("log h: %.3g relative to max(1, |log h|); log g: %.3g absolute; r: %.3g relative, over %d points" % (e_h, e_g, e_r, len(zs)))
    assert np.all(np.isfinite(lh)) and np.all(np.isfinite(r)) and np.all(r > 0)
    assert e_h <= 3e-15 and e_g <= 1e-12 and e_r <= 1e-12


def _exact_psi(t):
    with mp.workdps(DIGITS):
        t = mp.mpf(float(t))
        sp = mp.log(1 + mp.exp(t)) if t < 200 else t + mp.exp(-t)
        psi = sp + mp.mpf(1) / 10 / (1 + t * t)
        sig = 1 / (1 + mp.exp(-t))
        return mp.log(psi), (sig - mp.mpf(2) / 10 * t / (1 + t * t) ** 2) / psi


def test_log_psi_against_mpmath():
    ts = np.array(list(np.linspace(-60.0, 60.0, 481)) + [s * 10.0 ** k for k in range(2, 301) for s in (1.0, -1.0)])
    lp, ratio = LR.log_psi(ts)
    e_p = e_q = 0.0
    for t, a, b in zip(ts, lp, ratio):
        L, Q = _exact_psi(t)
        e_p = max(e_p, float(abs(a - L) / max(1, abs(L))))
        e_q = max(e_q, float(abs(b - Q) / abs(Q)))
    print("log psi: %.3g relative to max(1, |log psi|); psi' / psi: %.3g relative, over %d points" % (e_p, e_q, len(ts)))
    assert np.all(np.isfinite(lp)) and np.all(ratio > 0) and np.all(np.isfinite(ratio))        # psi is monotone, finite in log space
    assert np.all(np.diff(lp[:481]) > 0)
    assert e_p <= 1e-15 and e_q <= 2e-12
    # 0 < psi(t) - max(t, 0) <= ln 2 + 0.1, with equality at t = 0
    t = np.linspace(-50, 50, 2001)
    gap = np.exp(LR.log_psi(t)[0]) - np.maximum(t, 0.0)
    assert np.all(gap > 0) and gap.max() <= LR.BOUND * (1 + 1e-14) and abs(gap[1000] - LR.BOUND) < 1e-15


# ---- against the oracle's EI ---------------------------------------------------------------------------------------------------------
def _arrays(seed, m, n, N, scale=1.0, shift=0.0):
    rng = np.random.RandomState(seed)
    mean, var = scale * rng.uniform(-1, 1, size=(m, n)), scale ** 2 * rng.uniform(0.01, 0.5, size=(m, n))
    return rng, mean, var, scale * (rng.uniform(-1, 1, size=(m, N)) + shift)


def test_closed_form_is_the_log_of_the_oracles_ei():
    """exp(restatement) against oracle.cpu_ref.ma_acq wherever that exceeds 1e-280 (|log EI| <= 645, z >= -36).  The tolerance is the
    oracle's own error, per candidate: its phi and Phi each carry the rounding of the exponent z^2 / 2, (z^2 / 2) eps relative, and the sum
    u Phi + phi = phi (1 - |u| R) cancels to 1 / z^2 of its terms, so EI is off by (z^4 / 2) eps = 2 (log EI)^2 eps relative (z^2 = 2 |log EI|
    to leading order) -- 9e-11 at the far end; times 4, plus the restatement's gate on log h, 3e-15 |log EI|."""
    seen_small, worst = 0, 0.0
    for seed, shift in ((0, 0.0), (1, 2.0), (2, 6.0), (3, 12.0), (4, 16.0)):
        rng, mean, var, mu_train = _arrays(seed, 3, 60, 20, shift=shift)
        thetas = rng.uniform(0.2, 1.0, size=(2, 3))
        for prob in (None, np.array([0.3, 0.7])):
            ei = R.ma_acq(mean, var, mu_train, thetas, prob, "EI")[0][:, 0]
            lg = LR.log_linear([mean], [var], [LR.incumbents(mu_train, thetas)], thetas, prob)
            assert np.all(np.isfinite(lg))
            ok = ei > 1e-280
            if not ok.any():
                continue                                   # (the last shift: every EI below 1e-280, the log form finite all the same)
            seen_small += int(np.sum(ok & (ei < 1e-100)))
            le = np.abs(np.log(ei[ok]))
            rel = np.abs(np.exp(lg[ok]) - ei[ok]) / ei[ok]
            worst = max(worst, float(np.max(rel / (8.0 * le * le * np.finfo(float).eps + 3e-15 * np.maximum(le, 1.0)))))
            assert np.all(rel <= 8.0 * le * le * np.finfo(float).eps + 3e-15 * np.maximum(le, 1.0))
    print("closed form against the oracle's EI: worst error / bound %.3g" % worst)
    assert seen_small >= 10                                # (the comparison reaches deep into the tail)


@pytest.mark.parametrize("util", UTILS)
def test_monte_carlo_form_exceeds_the_oracles_ei_by_at_most_the_derived_bound(util):
    """0 < exp(log alpha_tau) - alpha_EI <= tau (ln 2 + 0.1).  The surplus of a sample far from the incumbent is 0.1 tau^3 / (U - best)^2:
    to be seen above the rounding of alpha_EI itself the posterior is scaled with tau, so that |U - best| stays within ~1e3 tau."""
    for tau in (1e-6, 1e-2, 1.0):
        quad, scales = util in ("neg_sq_dist", "rosenbrock"), util in ("linear", "neg_sq_dist", "rosenbrock")
        scale = (np.sqrt(tau) if quad else tau) * 10.0 if scales else 1.0
        rng, mean, var, mu_train = _arrays(7, 4, 40, 15, scale=scale)
        thetas, params = CR.utility_inputs(rng, util, 4, 3)
        if util in ("linear", "neg_sq_dist"):
            thetas = thetas * (1.0 if util == "linear" else scale)
        if util == "rosenbrock":
            thetas = thetas * scale
        W, prob = rng.normal(size=(30, 4)), rng.dirichlet(np.ones(3))
        if not scales and tau < 1.0:
            continue                                       # (utilities that do not scale: the surplus is below alpha_EI's rounding there)
        ei = R.mc_acq(mean, np.sqrt(var), mu_train, W, util, thetas, prob, "EI", params)[0][:, 0]
        lg = LR.log_mc([mean], [var], [LR.incumbents(mu_train, thetas, util, params)], W, thetas, prob, util, params, tau)
        diff = np.exp(lg) - ei
        print("%s tau %g: EI in [%.3g, %.3g], surplus / (tau (ln 2 + 0.1)) in [%.3g, %.3g]" % (util, tau, ei.min(), ei.max(), (diff / (tau * LR.BOUND)).min(),
                                                                                          (diff / (tau * LR.BOUND)).max()))
        assert np.all(np.isfinite(lg)) and np.all(diff > 0) and np.all(diff <= tau * LR.BOUND * (1 + 1e-12))


# ---- gradients against central differences of the value -------------------------------------------------------------------------------
def _small(util, seed=5, N=14, d=2, m=2, S=20, L=2, n=8, H=2):
    kinds = ["se", "matern52", "rbf", "matern32"][:m]
    X, Y, var, ls, nz, Xc = K.problem(kinds, N, d, n, seed, noise=1e-4)
    las = [K.LookAhead.fit(kinds, X, Y, var * (1 + 0.1 * h), ls * (1 - 0.05 * h), nz) for h in range(H)]
    rng = np.random.RandomState(100 + seed)
    thetas, params = CR.utility_inputs(rng, util, m, L)
    return las, Xc, rng.normal(size=(S, m)), thetas, rng.dirichlet(np.ones(L)), params


def _fd(f, Xc, h=1e-6):
    fd = np.zeros_like(Xc)
    for q in range(Xc.shape[1]):
        Xp, Xm = Xc.copy(), Xc.copy()
        Xp[:, q] += h
        Xm[:, q] -= h
        fd[:, q] = (f(Xp) - f(Xm)) / (2 * h)
    return fd


@pytest.mark.parametrize("shift", [0.0, 3.0, 40.0])
def test_closed_form_gradient_against_central_differences(shift):
    """rtol 1e-3, atol 1e-6 max(1, |g|max), the finite-difference gate of the other restatements; the incumbent raised by `shift` walks z from
    the bulk deep into the tail, where EI itself is an exact zero."""
    las, Xc, _, thetas, prob, _ = _small("linear")
    bests = [LR.incumbents(CR.train_mean(la), thetas) + shift for la in las]

    def value(X):
        post = [CR.posterior(la, X) for la in las]
        return LR.log_linear([p[0] for p in post], [p[1] for p in post], bests, thetas, prob)
    post = [CR.posterior(la, Xc, grad=True) for la in las]
    v, g = LR.log_linear([p[0] for p in post], [p[1] for p in post], bests, thetas, prob, [p[2] for p in post], [p[3] for p in post])
    fd = _fd(value, Xc)
    print("shift %g: log alpha in [%.4g, %.4g], gradient scale %.3g, max abs difference %.3g" % (shift, v.min(), v.max(), np.abs(g).max(), np.abs(g - fd).max()))
    assert np.all(np.isfinite(v)) and np.abs(g).max() > 0
    np.testing.assert_allclose(g, fd, rtol=1e-3, atol=1e-6 * max(1.0, np.abs(g).max()))


@pytest.mark.parametrize("tau", [1e-3, 1.0])
@pytest.mark.parametrize("util", UTILS)
def test_monte_carlo_gradient_against_central_differences(util, tau):
    las, Xc, W, thetas, prob, params = _small(util)
    bests = [LR.incumbents(CR.train_mean(las[0]), thetas, util, params) + 0.5] * len(las)

    def value(X):
        post = [CR.posterior(la, X) for la in las]
        return LR.log_mc([p[0] for p in post], [p[1] for p in post], bests, W, thetas, prob, util, params, tau)
    post = [CR.posterior(la, Xc, grad=True) for la in las]
    v, g = LR.log_mc([p[0] for p in post], [p[1] for p in post], bests, W, thetas, prob, util, params, tau, [p[2] for p in post], [p[3] for p in post])
    fd = _fd(value, Xc)
    print("%s tau %g: log alpha in [%.4g, %.4g], gradient scale %.3g, max abs difference %.3g" % (util, tau, v.min(), v.max(), np.abs(g).max(), np.abs(g - fd).max()))
    assert np.all(np.isfinite(v)) and np.abs(g).max() > 0
    np.testing.assert_allclose(g, fd, rtol=1e-3, atol=1e-6 * max(1.0, np.abs(g).max()))


def test_terms_without_weight_and_the_empty_mixture():
    rng, mean, var, mu_train = _arrays(3, 2, 5, 6)
    thetas = np.array([[0.5, 0.5], [0.0, 0.0], [0.2, 0.9]])
    best = LR.incumbents(mu_train, thetas)
    dm, dv = rng.normal(size=(2, 5, 3)), rng.normal(size=(2, 5, 3))
    full, g = LR.log_linear([mean], [var], [best], thetas, np.array([0.5, 0.5, 0.0]), [dm], [dv])
    only, g1 = LR.log_linear([mean], [var], [best[:1]], thetas[:1], np.array([0.5]), [dm], [dv])
    np.testing.assert_allclose(full, only, rtol=1e-15)     # theta = 0 (sigma = 0) and p = 0 are -inf terms: only the first is left
    np.testing.assert_allclose(g, g1, rtol=1e-14)
    v, g = LR.log_linear([mean], [var], [best[1:2]], thetas[1:2], None, [dm], [dv])
    assert np.all(v == -np.inf) and np.all(g == 0.0)
    v, g = LR.log_mc([mean], [var], [best[:1]], rng.normal(size=(4, 2)), thetas[:1], np.array([0.0]), "linear", None, 1.0, [dm], [dv])
    assert np.all(v == -np.inf) and np.all(g == 0.0)
    # two hyper-samples with the same posterior are one
    one = LR.log_linear([mean], [var], [best], thetas, None)
    np.testing.assert_allclose(LR.log_linear([mean, mean], [var, var], [best, best], thetas, None), one, rtol=1e-14)


# ---- surface -------------------------------------------------------------------------------------------------------------------------
def test_header_declares_and_library_exports_the_entry_points():
    header = open(os.path.join(ROOT, "include", "bocf_hip.h")).read()
    lib = _ffi.load()
    for name in ENTRY_POINTS:
        assert re.search(r"\bint %s\(bocf_ctx\* ctx" % name, header), name
        assert name in _ffi.SIGNATURES
        assert isinstance(getattr(lib, name), ctypes._CFuncPtr)
    from bocf_amd import build
    assert "logei.hip" in build.SOURCES and "capi_logei.hip" in build.SOURCES


def test_abi_refusals_that_need_no_gpu():
    lib, dp = _ffi.load(), _ffi.dptr
    th = np.zeros((1, 3))

    def bad(rc, name, text):
        msg = lib.bocf_last_error()
        assert rc < 0 and name.encode() in msg and text.encode() in msg, (rc, msg, text)
    who = "bocf_acq_log_mc"
    for tau in (0.0, -1.0, np.inf, np.nan):
        bad(lib.bocf_acq_log_mc(None, tau, _ffi.UTIL_NEG_SQ_DIST, None, 0, dp(th), 3, None, 1, None, None), who, "tau must be finite and > 0")
    bad(lib.bocf_acq_log_mc(None, 1.0, 7, None, 0, dp(th), 3, None, 1, None, None), who, "unknown utility kind")
    bad(lib.bocf_acq_log_mc(None, 1.0, -1, None, 0, dp(th), 3, None, 1, None, None), who, "unknown utility kind")
    bad(lib.bocf_acq_log_mc(None, 1.0, _ffi.UTIL_NEG_SQ_DIST, None, 0, dp(th), 3, None, 1, None, None), who, "model not fitted")
    bad(lib.bocf_acq_log_linear(None, dp(th), None, 1, None, None), "bocf_acq_log_linear", "model not fitted")


# ---- every argument check of the two entry points, through the stand-alone driver (bocf_amd/csrc/logei_args.h) -----------------------------
CLANG = "/opt/rocm/lib/llvm/bin/clang++"
CHECKS = ["tau must be finite and > 0", "unknown utility kind", "model not fitted", "not a whole number of hyper-samples", "option best_group",
          "more outputs per hyper-sample", "no Monte-Carlo samples set (bocf_set_mc_samples)", "L out of range", "theta must be", "theta_dim must equal m",
          "rosenbrock utility needs even m", "bad utility parameters", "neg_exp_cos needs m weights", "no resident candidates", "host-given posterior",
          "input dimension too large (gradients: d <= 64)"]
# one fault per check of bocf_acq_log_mc, in the order the entry point makes them
FAULTS = [dict(tau="0"), dict(kind=7), dict(fitted=0), dict(m=5, H=2), dict(best_group=1), dict(m=17, theta_dim=16, kind=2), dict(S_mc=0), dict(L=0),
          dict(theta_null=1), dict(theta_dim=3), dict(kind=4, theta_dim=1, m=3), dict(n_params=2), dict(kind=3, theta_dim=1), dict(C=0),
          dict(canned=1, grad=1), dict(d=65, grad=1)]


@pytest.fixture(scope="module", params=["plain", "sanitized"])
def driver(request, tmp_path_factory):
    assert os.path.exists(CLANG), "no clang++ next to hipcc"
    exe = str(tmp_path_factory.mktemp("logei_args") / ("logei_args_driver_" + request.param))
    extra = ["-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-g"] if request.param == "sanitized" else []
    subprocess.check_call([CLANG, "-std=c++17", "-O2", "-Wall", "-Werror"] + extra + [os.path.join(ROOT, "tests", "logei_args_driver.cpp"), "-o", exe])
    return exe


def _line(who, tau="1e-6", **kw):
    c = dict(fitted=1, canned=0, m=4, H=1, best_group=-1, S_mc=25, d=3, C=5, kind=1, n_params=0, params_null=1, theta_null=0, theta_dim=4, L=3, grad=0)
    c.update(kw)
    return ("%s|%d %d %d %d %d %d %d %d|%d %d %d %d %d %d %d|%s"
            % (who, c["fitted"], c["canned"], c["m"], c["H"], c["best_group"], c["S_mc"], c["d"], c["C"], c["kind"], c["n_params"], c["params_null"],
               c["theta_null"], c["theta_dim"], c["L"], c["grad"], tau))


def _verdicts(driver, lines):
    out = subprocess.run([driver], input="".join(l + "\n" for l in lines), capture_output=True, text=True)
    assert out.returncode == 0, out.stderr
    got = out.stdout.split("\n")[:-1]
    assert len(got) == len(lines), (got, out.stderr)
    return got


def test_each_refusal_names_the_entry_point_in_its_own_words(driver):
    who = "bocf_acq_log_mc"
    assert len(FAULTS) == len(CHECKS)
    for g, text, f in zip(_verdicts(driver, [_line(who, **f) for f in FAULTS]), CHECKS, FAULTS):
        assert g.startswith(who + ": ") and text in g, (f, g)
    bad_tau = [_line(who, tau=t) for t in ("0", "-1", "inf", "-inf", "nan")] + [_line(who, L=33), _line(who, kind=-1)]
    for g, text in zip(_verdicts(driver, bad_tau), ["tau must be finite and > 0"] * 5 + ["L out of range", "unknown utility kind"]):
        assert g.startswith(who + ": ") and text in g, g
    # what is accepted: any positive finite tau, the ends of every range, the value form on a host-given posterior and at any d, the gradient
    # form at d = 64, a program (left to the check of the resident one) with and without parameters
    ok = [_line(who), _line(who, tau="1e-300"), _line(who, tau="1e300"), _line(who, canned=1), _line(who, d=65), _line(who, d=64, grad=1), _line(who, m=8, H=2),
          _line(who, m=8, H=2, best_group=1), _line(who, m=16, theta_dim=16), _line(who, L=32), _line(who, L=1), _line(who, kind=4, theta_dim=1),
          _line(who, kind=3, theta_dim=1, n_params=4, params_null=0), _line(who, kind=5, theta_dim=7), _line(who, kind=5, theta_dim=0, theta_null=1)]
    assert _verdicts(driver, ok) == ["ok 4"] * 8 + ["ok 16"] + ["ok 4"] * 4 + ["ok 4 program"] * 2
    assert "theta is null" in _verdicts(driver, [_line(who, kind=5, theta_dim=2, theta_null=1)])[0]
    # the closed form: theta is (L, m), so there is no theta_dim to get wrong, no tau and no samples
    who = "bocf_acq_log_linear"
    bad = [(_line(who, "none", fitted=0), "model not fitted"), (_line(who, "none", m=5, H=2), "whole number of hyper-samples"),
           (_line(who, "none", best_group=1), "option best_group"), (_line(who, "none", m=17), "more outputs per hyper-sample"),
           (_line(who, "none", L=0), "L out of range"), (_line(who, "none", L=33), "L out of range"), (_line(who, "none", theta_null=1), "theta is null"),
           (_line(who, "none", C=0), "no resident candidates"), (_line(who, "none", canned=1, grad=1), "host-given posterior"),
           (_line(who, "none", d=65, grad=1), "input dimension too large (gradients: d <= 64)")]
    for (_, text), g in zip(bad, _verdicts(driver, [l for l, _ in bad])):
        assert g.startswith(who + ": ") and text in g, (text, g)
    ok = [_line(who, "none"), _line(who, "none", S_mc=0), _line(who, "none", canned=1), _line(who, "none", d=65), _line(who, "none", d=64, grad=1), _line(who, "none", L=32)]
    assert _verdicts(driver, ok) == ["ok 4"] * 6


def test_the_earlier_of_two_faults_is_reported(driver):
    who = "bocf_acq_log_mc"
    pairs = [(dict(tau="nan", kind=7), CHECKS[0]), (dict(kind=7, fitted=0), CHECKS[1]), (dict(fitted=0, L=0), CHECKS[2]), (dict(m=5, H=2, S_mc=0), CHECKS[3]),
             (dict(S_mc=0, L=0), CHECKS[6]), (dict(L=0, theta_null=1), CHECKS[7]), (dict(theta_dim=3, C=0), CHECKS[9]), (dict(C=0, d=65, grad=1), CHECKS[13]),
             (dict(canned=1, d=65, grad=1), CHECKS[14])]
    for (f, text), g in zip(pairs, _verdicts(driver, [_line(who, **f) for f, _ in pairs])):
        assert text in g, (f, g)


# ---- the classes, on a stub model -------------------------------------------------------------------------------------------------------
class _MockModel(object):
    analytical_gradient_prediction = True

    def __init__(self, m):
        self.output_dim, self.calls = m, []

    def number_of_hyps_samples(self):
        return 1

    def acq_linear(self, X, kind, thetas, prob, n_hyps=None):
        self.calls.append(("linear", np.array(thetas), None if prob is None else np.array(prob)))
        return np.atleast_2d(X).sum(1)

    def acq_linear_grad(self, X, kind, thetas, prob, n_hyps=None):
        self.calls.append(("linear_grad", np.array(thetas), None if prob is None else np.array(prob)))
        X = np.atleast_2d(X)
        return X.sum(1), np.ones(X.shape)

    def acq_mc(self, X, kind, util_kind, util_params, thetas, prob, W=None, fetch=True, n_hyps=None, program=None):
        return np.zeros(len(np.atleast_2d(X)))

    def acq_mc_grad(self, X, util_kind, util_params, thetas, prob, W=None, n_hyps=None, program=None):
        X = np.atleast_2d(X)
        return np.zeros(len(X)), np.zeros(X.shape)

    def acq_log_linear(self, X, thetas, prob, n_hyps=None, grad=False, fetch=True):
        self.calls.append(("log_linear", np.array(thetas), None if prob is None else np.array(prob), n_hyps, grad))
        X = np.atleast_2d(X)
        return (X.sum(1), np.ones(X.shape)) if grad else X.sum(1)

    def acq_log_mc(self, X, util_kind, util_params, thetas, prob, tau, W=None, n_hyps=None, grad=False, program=None, fetch=True):
        self.calls.append(("log_mc", util_kind, np.array(thetas), None if prob is None else np.array(prob), tau, np.array(W), grad, program))
        X = np.atleast_2d(X)
        return (X.sum(1), np.ones(X.shape)) if grad else X.sum(1)


class _NoLogModel(object):
    """A device model of before: it has acq_linear, not the log-space entries."""
    analytical_gradient_prediction = True
    output_dim = 3

    def number_of_hyps_samples(self):
        return 1

    def acq_linear(self, *a, **kw):
        raise AssertionError("not used")


def _draws(cls, model, U, X, **kw):
    np.random.seed(11)
    acq = cls(model, None, utility=U, **kw)
    acq._compute_acq(X)
    acq._compute_acq_withGradients(X)
    acq._compute_acq(X)
    return acq, np.random.uniform()


def test_exports_class_surface_and_rng_touchpoints():
    for name in ("maLogEI", "LogEI", "uLogEI"):
        cls = getattr(B, name)
        assert cls is getattr(B.acquisitions, name) and issubclass(cls, B.AcquisitionBase)
        assert cls.analytical_gradient_prediction is True and cls._device_refine is False
    assert issubclass(B.LogEI, B.maLogEI)
    for name in ("acq_log_linear", "acq_log_mc"):
        assert "log" in getattr(B.multi_outputGP, name).__doc__
    assert "units of the utility" in B.multi_outputGP.acq_log_mc.__doc__ and "UNITS OF THE UTILITY" in B.uLogEI.__doc__
    support = np.array([[0.2, 0.3, 0.5], [0.6, 0.1, 0.3]])
    X = np.random.RandomState(0).uniform(size=(4, 2))
    for full in (True, False):
        dist = lambda: B.ParameterDistribution(support=support if full else np.repeat(support, 10, 0), prob_dist=np.array([0.25, 0.75]) if full else None)
        # the closed form: the draws of maEI / EI, in the constructor and per call
        lin = lambda: B.Utility(parameter_dist=dist(), linear=True)
        for ref_cls, cls in ((B.maEI, B.maLogEI), (B.EI, B.LogEI)):
            a0, u0 = _draws(ref_cls, _MockModel(3), lin(), X)
            a1, u1 = _draws(cls, _MockModel(3), lin(), X)
            assert u0 == u1 and a0.n_hyps_samples == a1.n_hyps_samples
            np.testing.assert_array_equal(np.array(a0.utility_params_samples), np.array(a1.utility_params_samples))
            assert [c[0] for c in a1.model.calls] == ["log_linear"] * 3 and [c[4] for c in a1.model.calls] == [False, True, False]
            for c0, c1 in zip(a0.model.calls, a1.model.calls):
                np.testing.assert_array_equal(c0[1], c1[1])
                assert (c0[2] is None and c1[2] is None) or np.array_equal(c0[2], c1[2])
        # the Monte-Carlo form: the draws of uEI_noiseless; update_Z_samples redraws W alone
        comp = lambda: B.Utility(parameter_dist=dist(), device="neg_sq_dist")
        a0, u0 = _draws(B.uEI_noiseless, _MockModel(3), comp(), X)
        a1, u1 = _draws(B.uLogEI, _MockModel(3), comp(), X)
        assert u0 == u1
        np.testing.assert_array_equal(a0.W_samples, a1.W_samples)
        np.testing.assert_array_equal(np.array(a0.utility_params_samples), np.array(a1.utility_params_samples))
    # what reaches the model
    U = B.Utility(parameter_dist=B.ParameterDistribution(support=support, prob_dist=np.array([0.25, 0.75])), device="neg_sq_dist")
    model = _MockModel(3)
    acq = B.uLogEI(model, None, utility=U, tau=1e-3)
    assert acq.tau == 1e-3 and B.uLogEI(_MockModel(3), None, utility=U).tau == 1e-6 and acq.analytical_gradient_acq
    v = acq._compute_acq(X)
    ev = model.calls[-1]
    assert v.shape == (4, 1) and np.array_equal(v[:, 0], X.sum(1))
    assert ev[0] == "log_mc" and ev[1] == _ffi.UTIL_NEG_SQ_DIST and np.array_equal(ev[2], support) and np.array_equal(ev[3], [0.25, 0.75]) and ev[4] == 1e-3
    assert np.array_equal(ev[5], acq.W_samples) and ev[6] is False and ev[7] is None
    f, df = acq.acquisition_function_withGradients(X)
    assert model.calls[-1][6] is True and np.array_equal(f[:, 0], -X.sum(1)) and np.array_equal(df, -np.ones(X.shape))
    for tau in (0.0, -1.0, np.inf, np.nan):
        with pytest.raises(ValueError, match="tau"):
            B.uLogEI(_MockModel(3), None, utility=U, tau=tau)
    # a utility program goes to the device with its blob
    prog = B.Utility(func=lambda t, y: -np.sum(np.square((y.transpose() - t).transpose()), axis=0), parameter_dist=B.ParameterDistribution(support=support, prob_dist=np.array([0.25, 0.75])),
                     device="program")
    model = _MockModel(3)
    B.uLogEI(model, None, utility=prog)._compute_acq(X)
    assert model.calls[-1][1] == _ffi.UTIL_PROGRAM and model.calls[-1][7] == prog.program_blob
    # no host fallback; the error names the way out
    odd = B.uLogEI(_MockModel(3), None, utility=B.Utility(func=lambda t, y: -np.sum(np.abs(y)), dfunc=lambda t, y: -np.sign(y),
                                                         parameter_dist=B.ParameterDistribution(support=support[:1], prob_dist=np.array([1.0]))))
    for call in (odd._compute_acq, odd._compute_acq_withGradients):
        with pytest.raises(NotImplementedError, match=r"Utility\(\.\.\., device=\.\.\."):
            call(X)
    lin = B.Utility(parameter_dist=B.ParameterDistribution(support=support, prob_dist=np.array([0.25, 0.75])), linear=True)
    for cls, U_ in ((B.maLogEI, lin), (B.LogEI, lin), (B.uLogEI, U)):
        with pytest.raises(TypeError):
            cls(_NoLogModel(), None, utility=U_)._compute_acq(X)           # not a device model with the entry point
        with pytest.raises(NotImplementedError, match="refine='device' does not cover %s" % cls.__name__):
            cls(_MockModel(3), None, utility=U_).device_refine_objective()
    assert B.LogEI(_MockModel(1), None, utility=B.Utility(parameter_dist=B.ParameterDistribution(support=np.array([[1.0]]), prob_dist=np.array([1.0])),
                                                          linear=True)).n_hyps_samples == 1
