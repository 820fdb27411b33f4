"""CPU checks of the joint q-point expected improvement (q-uEI): the NumPy restatement tests/joint_ref.py against central differences of
its own value and against one-line formulas, bocf_amd/csrc/joint_chol.h through a stand-alone driver built with the host compiler under
AddressSanitizer and UBSan, the caps of the device test's cases, and the Python layer's own refusals and host logic on a mock model."""
import ctypes
import os
import re
import shutil
import subprocess
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import joint_ref as J  # noqa: E402
import kg_ref as K  # noqa: E402
import pending_ref as PR  # noqa: E402

import bocf_amd as B  # noqa: E402
from bocf_amd import _ffi  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _small(q, seed, S=32, L=2, nb=3):
    kinds = ["se", "matern52"]
    X, Y, var, ls, nz, Xc = K.problem(kinds, 12, 3, nb * q, seed, noise=1e-4)
    la = K.LookAhead.fit(kinds, X, Y, var, ls, nz)
    rng = np.random.RandomState(100 + seed)
    Z, thetas = rng.normal(size=(S, 2, q)), rng.uniform(-0.5, 0.5, size=(L, 2))
    prob = rng.dirichlet(np.ones(L))
    Xb = Xc.reshape(nb, q, 3)
    best = J.median_best([la], Xb[0], Z, thetas, "neg_sq_dist")[0]
    return la, Xb, Z, thetas, prob, best


# ---- the restatement against itself ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("q", [1, 3, 8])
def test_gradient_against_central_differences(q):
    """Gate: 1e-6 relative to max|gradient| with h = 1e-6, on the batches no sample of which sits within 1e-4 scale of a kink (a step of
    h moves a utility by h x slope, slopes are O(10) here)."""
    la, Xb, Z, thetas, prob, best = _small(q, 40 + q)
    r = J.joint(la, Xb, Z, thetas, prob, "neg_sq_dist", best=best, grad=True)
    keep = np.flatnonzero((r["margin"] > 1e-4 * r["scale"]) & (r["alpha"] > 0))
    assert len(keep) >= 2 and r["floored"].sum() == 0
    h = 1e-6
    fd = np.zeros_like(r["dalpha"])
    for a in range(q):
        for x in range(3):
            Xp, Xm = Xb[keep].copy(), Xb[keep].copy()
            Xp[:, a, x] += h
            Xm[:, a, x] -= h
            fd[keep, a, x] = (J.joint(la, Xp, Z, thetas, prob, "neg_sq_dist", best=best)["alpha"]
                              - J.joint(la, Xm, Z, thetas, prob, "neg_sq_dist", best=best)["alpha"]) / (2 * h)
    gmax = np.abs(r["dalpha"][keep]).max()
    err = np.abs(r["dalpha"][keep] - fd[keep]).max()
    print("q = %d: gradient vs central differences on %d of %d batches: max abs difference %.3g, max |gradient| %.3g" % (q, len(keep), len(Xb), err, gmax))
    assert gmax > 0 and err <= 1e-6 * gmax


def test_q1_is_the_one_line_formula():
    la, Xb, Z, thetas, prob, best = _small(1, 3, nb=5)
    r = J.joint(la, Xb, Z, thetas, prob, "neg_sq_dist", best=best)
    x = Xb[:, 0, :]
    mu = la.mean(x)
    for b in range(len(x)):
        s2b = np.array([la.cov(x[b:b + 1], x[b:b + 1])[j, 0, 0] for j in range(2)])
        sd = np.sqrt(s2b + 1e-8 * np.maximum(s2b, 1e-10))
        y = mu[:, b][None, :] + sd[None, :] * Z[:, :, 0]                                   # (S, m)
        one = sum(prob[l] * np.mean(np.maximum(-np.sum((y - thetas[l]) ** 2, 1) - best[l], 0.0)) for l in range(len(thetas)))
        np.testing.assert_allclose(r["alpha"][b], one, rtol=1e-12, atol=1e-15)


def test_alpha_does_not_decrease_when_best_decreases():
    la, Xb, Z, thetas, prob, best = _small(3, 5, nb=4)
    prev = None
    for shift in (0.5, 0.1, 0.0, -0.1, -0.5):
        a = J.joint(la, Xb, Z, thetas, prob, "neg_sq_dist", best=best + shift)["alpha"]
        assert np.all(a >= 0)
        if prev is not None:
            assert np.all(a >= prev)
        prev = a
    assert np.all(prev > 0)


def test_hyper_average_and_default_incumbent():
    la, Xb, Z, thetas, prob, best = _small(2, 6)
    one = J.joint(la, Xb, Z, thetas, prob, "neg_sq_dist", best=best)
    two = J.joint_hyper([la, la], Xb, Z, thetas, prob, "neg_sq_dist", best=best)
    np.testing.assert_allclose(two["alpha"], one["alpha"], rtol=1e-15)
    np.testing.assert_array_equal(two["floored"], 2 * one["floored"])
    d0 = J.joint(la, Xb, Z, thetas, prob, "neg_sq_dist")
    np.testing.assert_array_equal(d0["best"], PR.best_so_far(la, thetas, "neg_sq_dist"))


@pytest.mark.parametrize("case", J.CASES + J.CHUNK_CASES, ids=[J.case_id(c) for c in J.CASES + J.CHUNK_CASES])
def test_caps_of_the_device_cases(case):
    """What tests/test_gpu_joint.py asserts on the restatement before it looks at the device, checked here where a seed can be changed."""
    inp = J.case_inputs(*case)
    las = PR.case_lookaheads(inp)
    ref, _ = J.case_reference(inp, las)
    nb = len(ref["alpha"])
    print("%s: cond %.3g, scale %.3g, near a kink %d of %d, alpha > 0 on %d, floored %d" % (J.case_id(case), ref["cond"], ref["scale"],
          np.sum(ref["margin"] <= 1e-6 * ref["scale"]), nb, np.sum(ref["alpha"] > 1e-6 * ref["scale"]), ref["floored"].sum()))
    assert ref["cond"] <= 1e4
    assert np.sum(ref["margin"] <= 1e-6 * ref["scale"]) <= nb / 8.0
    assert np.sum(ref["alpha"] > 1e-6 * ref["scale"]) >= 0.75 * nb
    assert ref["floored"].sum() == 0


# ---- joint_chol.h through the stand-alone driver ---------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def driver(tmp_path_factory):
    cxx = shutil.which("g++") or shutil.which("clang++")
    assert cxx, "no host C++ compiler"
    exe = str(tmp_path_factory.mktemp("joint") / "joint_chol_driver")
    subprocess.check_call([cxx, "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-o", exe,
                           os.path.join(ROOT, "tests", "joint_chol_driver.cpp")])
    return exe


def _run_driver(exe, records):
    """records: [(A (q, q), Cbar (q, q), use_tau)] -> [(tau, floored (q,) bool, C, G lower)]"""
    text = "%d\n" % len(records)
    for A, Cb, use_tau in records:
        text += "%d %d\n" % (len(A), int(use_tau)) + "\n".join("%.17g" % v for a in (A, Cb) for v in np.ravel(a)) + "\n"
    out = subprocess.run([exe], input=text, capture_output=True, text=True)
    assert out.returncode == 0, out.stderr
    v, res = out.stdout.split(), []
    for A, _, _ in records:
        q = len(A)
        tau, mask = float(v[0]), int(v[1])
        C = np.array(v[2:2 + q * q], dtype=float).reshape(q, q)
        G = np.array(v[2 + q * q:2 + 2 * q * q], dtype=float).reshape(q, q)
        v = v[2 + 2 * q * q:]
        res.append((tau, np.array([(mask >> k) & 1 for k in range(q)], dtype=bool), C, G))
    assert not v
    return res


def _sym(G):
    low = np.tril(G, -1)
    return np.diag(np.diag(G)) + 0.5 * (low + low.T)


def _spd(rng, q, scale):
    A = rng.normal(size=(q, q + 2))
    return scale * (A.dot(A.T) / (q + 2) + 0.05 * np.eye(q))


def test_driver_factor_and_adjoint_against_the_restatement(driver):
    """Random SPD 1 x 1 .. 8 x 8 matrices at three scales: the factor against NumPy's and the restatement's to a few ulps x cond, the
    reverse pass against the restatement's."""
    rng = np.random.RandomState(0)
    recs = [(_spd(rng, q, 10.0 ** e), rng.normal(size=(q, q)), True) for q in range(1, 9) for e in (-3, 0, 2)]
    for (A, Cb, _), (tau, floored, C, G) in zip(recs, _run_driver(driver, recs)):
        q = len(A)
        assert abs(tau - J.jitter(A)) <= 8 * np.finfo(float).eps * tau and not floored.any()     # (NumPy sums the q <= 8 diagonal entries in another order)
        Cr, fr = J.chol_floor(A, tau)
        cond = np.linalg.cond(A + tau * np.eye(q))
        np.testing.assert_allclose(C, np.linalg.cholesky(A + tau * np.eye(q)), rtol=0, atol=8 * np.finfo(float).eps * cond * np.abs(Cr).max())
        np.testing.assert_allclose(C, Cr, rtol=0, atol=8 * np.finfo(float).eps * cond * np.abs(Cr).max())
        assert np.all(np.triu(C, 1) == 0) and np.all(np.triu(G, 1) == 0)
        Sr = J.chol_adjoint(Cr, fr, Cb)
        np.testing.assert_allclose(_sym(G), Sr, rtol=0, atol=64 * np.finfo(float).eps * cond * np.abs(Sr).max())


def test_driver_floored_paths(driver):
    """A zero matrix floors every pivot, a rank-1 matrix all but the first (no jitter: tau = 0); the adjoints of floored pivots are dropped
    and everything stays finite."""
    v = np.array([1.0, -2.0, 0.5, 3.0])
    zero, rank1 = np.zeros((4, 4)), np.outer(v, v)
    Cb = np.random.RandomState(1).normal(size=(4, 4))
    (t0, f0, C0, G0), (t1, f1, C1, G1) = _run_driver(driver, [(zero, Cb, False), (rank1, Cb, False)])
    assert t0 == 0 and f0.all() and np.array_equal(C0, np.sqrt(1e-10) * np.eye(4))
    assert np.array_equal(np.diag(G0), np.zeros(4)) and np.all(np.isfinite(G0))
    assert list(f1) == [False, True, True, True]
    np.testing.assert_allclose(C1[:, 0], v, rtol=1e-15)
    np.testing.assert_allclose(np.diag(C1)[1:], np.sqrt(1e-10), rtol=1e-15)
    assert np.all(np.isfinite(G1)) and np.all(np.diag(G1)[1:] == 0)
    for A, f, C, G in ((zero, f0, C0, G0), (rank1, f1, C1, G1)):
        Cr, fr = J.chol_floor(A, 0.0)
        assert np.array_equal(fr, f)
        np.testing.assert_allclose(C, Cr, rtol=1e-13, atol=1e-18)
        np.testing.assert_allclose(_sym(G), J.chol_adjoint(Cr, fr, Cb), rtol=1e-9, atol=1e-9 * np.abs(G).max())


@pytest.mark.parametrize("q", [1, 2, 5, 8])
def test_driver_adjoint_against_differences_of_the_factor(driver, q):
    """sum(Cbar o dC) for a symmetric perturbation dA of A equals sum(Sigmabar o dA): central differences of the driver's own factor."""
    rng = np.random.RandomState(10 + q)
    A, Cb = _spd(rng, q, 1.0), np.tril(rng.normal(size=(q, q)))
    D = rng.normal(size=(q, q))
    D = 0.5 * (D + D.T)
    h = 1e-6
    (_, _, _, G), (_, _, Cp, _), (_, _, Cm, _) = _run_driver(driver, [(A, Cb, False), (A + h * D, Cb, False), (A - h * D, Cb, False)])
    fd = np.sum(Cb * (Cp - Cm)) / (2 * h)
    an = np.sum(_sym(G) * D)
    assert abs(fd - an) <= 1e-7 * max(abs(an), np.abs(G).max())


# ---- surface and host logic ------------------------------------------------------------------------------------------------------
def test_header_declares_and_library_exports_the_entry_point():
    header = open(os.path.join(ROOT, "include", "bocf_hip.h")).read()
    lib = _ffi.load()
    assert re.search(r"\bint bocf_acq_joint\(bocf_ctx\* ctx", header)
    assert "bocf_acq_joint" in _ffi.SIGNATURES and isinstance(lib.bocf_acq_joint, ctypes._CFuncPtr)
    assert lib.bocf_acq_joint(None, 2, None, 1, 1, None, 0, None, 0, None, 1, None, None, None, None) < 0 and b"bocf_acq_joint" in lib.bocf_last_error()
    from bocf_amd import build
    assert "joint.hip" in build.SOURCES and "capi_joint.hip" in build.SOURCES
    assert B.uEI_joint is B.acquisitions.uEI_joint and B.CompositeJointBatch is B.cbo.CompositeJointBatch
    assert B.multi_outputGP.acq_joint.__doc__ and B.uEI_joint.analytical_gradient_prediction is True


def test_model_refusals_need_no_device():
    model = B.multi_outputGP(2, fixed_hyps=True)
    Z = np.zeros((4, 2, 3))
    for q in (0, 9):
        with pytest.raises(ValueError, match="q must be"):
            model.acq_joint(np.zeros((1, 6)), q, _ffi.UTIL_NEG_SQ_DIST, None, np.zeros((1, 2)), None, Z)
    for bad in (np.zeros((4, 2, 2)), np.zeros((4, 3, 3)), np.zeros((4, 6)), np.zeros((257, 2, 3)), np.zeros((0, 2, 3))):
        with pytest.raises(ValueError, match="Z must be"):
            model.acq_joint(np.zeros((1, 6)), 3, _ffi.UTIL_NEG_SQ_DIST, None, np.zeros((1, 2)), None, bad)
    with pytest.raises(RuntimeError, match="no model yet"):
        model.acq_joint(np.zeros((1, 6)), 3, _ffi.UTIL_NEG_SQ_DIST, None, np.zeros((1, 2)), None, Z)
    model._X = np.zeros((5, 2))                       # (a shape is all the remaining checks read)
    for bad in (np.zeros((1, 5)), np.zeros((0, 6)), np.zeros((2, 2, 2))):
        with pytest.raises(ValueError, match="whole batches"):
            model.acq_joint(bad, 3, _ffi.UTIL_NEG_SQ_DIST, None, np.zeros((1, 2)), None, Z)
    with pytest.raises(ValueError, match="at most 128 points"):
        model.acq_joint(np.zeros((43, 6)), 3, _ffi.UTIL_NEG_SQ_DIST, None, np.zeros((1, 2)), None, Z, grad=True)


class _MockModel(object):
    analytical_gradient_prediction = True

    def __init__(self, m, d):
        self.output_dim, self.d, self.calls = m, d, []

    def number_of_hyps_samples(self):
        return 1

    def acq_joint(self, X, q, util_kind, util_params, thetas, prob, Z, n_hyps=None, best=None, grad=False):
        X = np.asarray(X, dtype=float)
        self.calls.append((X.shape, q, util_kind, np.array(thetas), None if prob is None else np.array(prob), np.array(Z), grad))
        v = -np.sum((X - 0.3) ** 2, 1)
        return (v, (-2.0 * (X - 0.3)).reshape(len(X), q, -1)) if grad else v


def _utility(m=2):
    support = np.array([[0.2, 0.3], [0.6, 0.1]])[:, :m]
    return B.Utility(parameter_dist=B.ParameterDistribution(support=support, prob_dist=np.array([0.25, 0.75])), device="neg_sq_dist"), support


def test_uei_joint_host_logic_and_draw_order():
    U, support = _utility()
    model = _MockModel(2, 2)
    np.random.seed(3)
    acq = B.uEI_joint(model, None, utility=U, q=3, n_samples=7)
    np.random.seed(3)
    W = np.random.normal(size=(25, 2))
    Zs = np.random.normal(size=(7, 2, 3))
    np.testing.assert_array_equal(acq.W_samples, W)
    np.testing.assert_array_equal(acq.Z_samples, Zs)
    state = np.random.get_state()
    acq.update_Z_samples(5)
    np.random.set_state(state)
    np.testing.assert_array_equal(acq.Z_samples, np.random.normal(size=(5, 2, 3)))
    X = np.random.RandomState(0).uniform(size=(50, 6))
    v = acq._compute_acq(X)
    assert v.shape == (50, 1) and len(model.calls) == 1
    shape, q, kind, th, pr, Z, grad = model.calls[0]
    assert shape == (50, 6) and q == 3 and kind == _ffi.UTIL_NEG_SQ_DIST and not grad
    assert np.array_equal(th, support) and np.array_equal(pr, [0.25, 0.75]) and np.array_equal(Z, acq.Z_samples)
    v2, g = acq._compute_acq_withGradients(X)                          # 50 batches of 3 points: groups of 42 and 8
    assert v2.shape == (50, 1) and g.shape == (50, 6) and np.array_equal(v2, v)
    np.testing.assert_array_equal(g, -2.0 * (X - 0.3))
    assert [c[0] for c in model.calls[1:]] == [(42, 6), (8, 6)] and all(c[6] for c in model.calls[1:])
    f, df = acq.acquisition_function_withGradients(X[:2])
    assert np.array_equal(f, -v[:2]) and np.array_equal(df, -g[:2])
    with pytest.raises(ValueError, match="multiple of q"):
        acq._compute_acq(np.zeros((1, 5)))
    for bad in (dict(q=0), dict(q=9), dict(n_samples=0), dict(n_samples=257)):
        with pytest.raises(ValueError):
            B.uEI_joint(model, None, utility=U, **bad)
    with pytest.raises(ValueError):
        acq.update_Z_samples(300)
    # a utility without a compiled-in device kind, and a traced program
    dist = B.ParameterDistribution(support=np.array([[0.1, 0.2]]), prob_dist=np.array([1.0]))
    host = B.Utility(func=lambda t, y: -np.sum(np.abs(y)), dfunc=lambda t, y: -np.sign(y), parameter_dist=dist)
    odd = B.uEI_joint(_MockModel(2, 2), None, utility=host, q=2)
    with pytest.raises(NotImplementedError, match="device kind"):
        odd._compute_acq(np.zeros((1, 4)))
    with pytest.raises(NotImplementedError, match="device kind"):
        odd._compute_acq_withGradients(np.zeros((1, 4)))


class _WarmStart(object):
    def __init__(self, X):
        self.X, self.calls = X, 0

    def compute_batch(self, duplicate_manager=None, context_manager=None, x_baseline=None):
        self.calls += 1
        np.random.uniform()
        return self.X


def test_joint_batch_draw_order_anchors_and_result():
    U, _ = _utility()
    d, q = 2, 3
    model = _MockModel(2, d)
    np.random.seed(8)
    acq = B.uEI_joint(model, [(0.0, 1.0)] * d, utility=U, q=q, n_samples=4)
    warm = _WarmStart(np.full((q, d), 0.9))
    ev = B.CompositeJointBatch(acq, q, n_starting=20, n_anchor=4, warm_start=warm)
    state = np.random.get_state()
    X = ev.compute_batch()
    after = np.random.uniform()
    # the draws: q * d uniform columns of the starting design, then the warm start's
    np.random.set_state(state)
    starts = np.stack([np.random.uniform(0.0, 1.0, size=20) for _ in range(q * d)], 1)
    np.random.uniform()
    assert np.random.uniform() == after and warm.calls == 1
    info = ev.last_info
    order = np.argsort(np.sum((starts - 0.3) ** 2, 1), kind="stable")[:4]
    np.testing.assert_array_equal(info["anchors"][:4], starts[order])
    np.testing.assert_array_equal(info["anchors"][4], np.full(q * d, 0.9))
    assert X.shape == (q, d) and np.all(X >= 0) and np.all(X <= 1)
    np.testing.assert_allclose(X, 0.3, atol=1e-5)                      # the mock's maximiser
    assert info["value"] >= info["anchor_values"].max() and info["value"] == info["refined_values"].max()
    # refusals
    with pytest.raises(ValueError):
        B.CompositeJointBatch(acq, 9)
    with pytest.raises(TypeError):
        B.CompositeJointBatch(acq, 2)                                   # q of the acquisition is 3
    with pytest.raises(TypeError):
        B.CompositeJointBatch(object(), 3)
    with pytest.raises(ValueError):
        B.CompositeJointBatch(acq, 3, n_starting=4, n_anchor=5)
    with pytest.raises(TypeError):
        B.CompositeJointBatch(acq, 3, warm_start=object())
    with pytest.raises(ValueError, match="warm_start returned"):
        B.CompositeJointBatch(acq, 3, n_starting=4, n_anchor=2, warm_start=_WarmStart(np.zeros((2, d)))).compute_batch()
