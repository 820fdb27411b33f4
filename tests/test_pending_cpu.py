"""Pending-point acquisition, CPU side: the NumPy restatement (tests/pending_ref.py) -- its two routes against each other, the increment
identity alpha(x | P) + qEI(P) = qEI(P u {x}) by brute force, its gradient against central differences --, the host arithmetic
(bocf_amd/csrc/pending_host.h through a sanitized stand-alone driver), the public surface, the host logic of uEI_pending and
CompositeGreedyBatch on a mock device model, and the seeds of the device test's cases."""
import ctypes
import os
import re
import shutil
import subprocess
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import kg_ref as K  # noqa: E402
import pending_ref as PR  # noqa: E402

import bocf_amd as B  # noqa: E402
from bocf_amd import _ffi  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENTRY_POINTS = ["bocf_set_pending_points", "bocf_get_pending_samples", "bocf_acq_pending"]


def _small(kind, seed=3, N=14, d=2, m=2, r=3, S=40, L=2, n=12):
    """A small problem.  Returns also `best`: the MINIMUM over the training inputs of U(theta_l, mu(X_i)) instead of the maximum the
    acquisitions use (the restatement takes it as an input): the thresholds are then mostly those of the pending samples, a sample at x
    beats them about once in r + 1 times, and every term of the sums is exercised."""
    kinds = ["se", "matern52", "rbf", "matern32"][:m]
    X, Y, var, ls, nz, Xc = K.problem(kinds, N, d, n, seed, noise=1e-4)
    la = K.LookAhead.fit(kinds, X, Y, var, ls, nz)
    rng = np.random.RandomState(seed)
    P = rng.uniform(size=(r, d))
    Zp, W = rng.normal(size=(S, m, r)), rng.normal(size=(S, m))
    thetas = rng.uniform(0.2, 1.0, size=(L, 1)) if kind == "rosenbrock" else (np.zeros((L, 1)) if kind in ("neg_sum_exp", "neg_exp_cos")
                                                                              else rng.uniform(-0.5, 0.5, size=(L, m)))
    prob = rng.dirichlet(np.ones(L))
    params = rng.uniform(0.5, 1.0, size=m) if kind == "neg_exp_cos" else None
    best = np.array([np.min(PR.R.utility_eval(kind, th, la.mean(X), params)) for th in thetas])
    return la, Xc, P, Zp, W, thetas, prob, params, best


# ---- the restatement ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", PR.CASES, ids=lambda c: "N%d-d%d-m%d-r%d-S%d-L%d-H%d-C%d-%s" % c[:9])
def test_device_cases_two_routes_and_seeds(case):
    """For every case of the device test, on its fixed seed: the bordered-Cholesky route and the conditional route of the restatement
    agree (their largest difference is printed: the floor a device case may refer to), cond(Sigma~) <= 1e4, and at most 5 % of the
    candidates have a sample within 1e-6 scale of its threshold.  A seed that fails is replaced in pending_ref.SEEDS."""
    inp = PR.case_inputs(*case)
    las = PR.case_lookaheads(inp)
    a = PR.case_reference(inp, las)
    b = PR.case_reference(inp, las, route="conditional")
    diff = float(np.max(np.abs(a["alpha"] - b["alpha"])))
    near = float(np.mean(a["gap"] < 1e-6 * a["scale"]))
    print("case %r: two-route difference %.3g (scale %.3g), cond %.3g, near-threshold share %.3f, share with alpha > 0 %.2f, max alpha %.3g"
          % (case, diff, a["scale"], a["cond"], near, np.mean(a["alpha"] > 0), a["alpha"].max()))
    # both routes are backward-stable factorizations of the same matrices: eps cond(Sigma~) relative in y, so in alpha at most that x scale
    assert diff <= 100 * np.finfo(float).eps * a["cond"] * a["scale"]
    assert a["cond"] <= 1e4
    assert near <= 0.05
    assert np.any(a["alpha"] > 1e-9 * a["scale"]), "no candidate improves for this seed: choose another"


@pytest.mark.parametrize("kind", ["neg_sq_dist", "neg_sum_exp", "neg_exp_cos", "rosenbrock"])
def test_two_routes_agree_values_and_gradients(kind):
    la, Xc, P, Zp, W, thetas, prob, params, best = _small(kind)
    a = PR.pending(la, Xc, P, Zp, W, thetas, prob, kind, params, best=best, grad=True)
    b = PR.pending(la, Xc, P, Zp, W, thetas, prob, kind, params, best=best, grad=True, route="conditional")
    assert np.any(a["alpha"] > 0)
    print("%s: two routes differ by %.3g in alpha (max %.3g), %.3g in the gradient (max %.3g)"
          % (kind, np.abs(a["alpha"] - b["alpha"]).max(), a["alpha"].max(), np.abs(a["dalpha"] - b["dalpha"]).max(), np.abs(a["dalpha"]).max()))
    np.testing.assert_allclose(a["alpha"], b["alpha"], rtol=1e-9, atol=1e-12 * a["scale"])
    np.testing.assert_allclose(a["dalpha"], b["dalpha"], rtol=1e-8, atol=1e-10 * np.abs(a["dalpha"]).max())
    np.testing.assert_array_equal(a["F"], b["F"])


@pytest.mark.parametrize("kind", ["neg_sq_dist", "neg_exp_cos"])
def test_increment_identity_by_brute_force(kind):
    """alpha(x | P) + qEI(P) = qEI(P u {x}) with the same normals: the joint normals of P u {x} are (Zp, W), the jitter of the
    conditional construction sits on the pending points' diagonal."""
    la, Xc, P, Zp, W, thetas, prob, params, best = _small(kind)
    res = PR.pending(la, Xc, P, Zp, W, thetas, prob, kind, params, best=best)
    r = len(P)
    tau = res["tau"]
    base = PR.qei(la, P, Zp, thetas, prob, kind, params, best, np.repeat(tau[:, None], r, 1))
    Z = np.concatenate([Zp, W[:, :, None]], 2)
    diag = np.concatenate([np.repeat(tau[:, None], r, 1), np.zeros((la.m, 1))], 1)
    joint = np.array([PR.qei(la, np.concatenate([P, x[None]]), Z, thetas, prob, kind, params, best, diag) for x in Xc])
    assert base > 0 and np.any(res["alpha"] > 0)
    np.testing.assert_allclose(res["alpha"] + base, joint, rtol=1e-9, atol=1e-12 * res["scale"])


@pytest.mark.parametrize("kind", ["neg_sq_dist", "neg_sum_exp", "neg_exp_cos", "rosenbrock"])
def test_gradient_against_central_differences(kind):
    """The restatement's gradient against central differences of its own value, on the candidates where no sample can cross its
    threshold within the step: gap > 2 h slope (slope: the largest l1 norm of a sample utility's x-gradient)."""
    la, Xc, P, Zp, W, thetas, prob, params, best = _small(kind, seed=5)
    r = PR.pending(la, Xc, P, Zp, W, thetas, prob, kind, params, best=best, grad=True)
    h = 1e-6
    keep = (r["gap"] > 4 * h * r["slope"]) & (r["alpha"] > 0)
    assert keep.sum() >= 4
    fd = np.zeros_like(Xc)
    for q in range(Xc.shape[1]):
        Xp, Xm = Xc.copy(), Xc.copy()
        Xp[:, q] += h
        Xm[:, q] -= h
        fd[:, q] = (PR.pending(la, Xp, P, Zp, W, thetas, prob, kind, params, best=best)["alpha"]
                    - PR.pending(la, Xm, P, Zp, W, thetas, prob, kind, params, best=best)["alpha"]) / (2 * h)
    # floor: posterior quantities carry ~ eps sqrt(cond(Ky)) of relative error (cond(Ky) <= (N sigma_f^2 + nugget) / nugget, N = 14,
    # sigma_f^2 <= 1.6, nugget 1e-4), a difference of utilities of size `scale` carries that / h
    atol = np.finfo(float).eps * np.sqrt((14 * 1.6 + 1e-4) / 1e-4) * r["scale"] / h
    print("%s: gradient vs central differences on %d of %d candidates: max abs difference %.3g, gradient scale %.3g, floor %.3g"
          % (kind, keep.sum(), len(Xc), np.abs(r["dalpha"][keep] - fd[keep]).max(), np.abs(fd[keep]).max(), atol))
    np.testing.assert_allclose(r["dalpha"][keep], fd[keep], rtol=1e-5, atol=atol)


# ---- pending_host.h through the stand-alone driver -------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def driver(tmp_path_factory):
    cxx = shutil.which("g++") or shutil.which("clang++")
    assert cxx, "no host C++ compiler"
    exe = str(tmp_path_factory.mktemp("pending") / "pending_host_driver")
    subprocess.check_call([cxx, "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-o", exe,
                           os.path.join(ROOT, "tests", "pending_host_driver.cpp")])
    return exe


def _run_driver(exe, Sigma, mu, Zp, m, tries):
    M, r = mu.shape
    S = Zp.shape[0]
    text = "%d %d %d %d %d\n" % (M, m, r, S, tries) + "\n".join("%.17g" % v for a in (Sigma, mu, Zp) for v in np.ravel(a)) + "\n"
    out = subprocess.run([exe], input=text, capture_output=True, text=True)
    assert out.returncode == 0, out.stderr
    v = np.array(out.stdout.split(), dtype=float)
    rc, v = int(v[0]), v[1:]
    sizes = [M, M * r * r, M * r * r, M * r * S, M * r * S]
    parts = np.split(v, np.cumsum(sizes)[:-1])
    return rc, parts[0], parts[1].reshape(M, r, r), parts[2].reshape(M, r, r), parts[3].reshape(M, r, S), parts[4].reshape(M, r, S)


def _spd(rng, r, scale):
    A = rng.normal(size=(r, r + 2))
    return scale * (A.dot(A.T) / (r + 2) + 0.05 * np.eye(r))


@pytest.mark.parametrize("r", [1, 7, 15])
def test_host_arithmetic_against_numpy(driver, r):
    """tau, L, Q, F, G of M = 2 hyper-samples x m = 3 outputs against NumPy (ladder rung 0 holds for these matrices)."""
    rng = np.random.RandomState(r)
    m, H, S = 3, 2, 5
    M = m * H
    Sigma = np.stack([_spd(rng, r, 10.0 ** (j - 2)) for j in range(M)])
    mu, Zp = rng.normal(size=(M, r)), rng.normal(size=(S, m, r))
    rc, tau, L, Q, F, G = _run_driver(driver, Sigma, mu, Zp, m, 10)
    assert rc == 0
    for j in range(M):
        t, Lr = PR.ladder(Sigma[j], 10)
        assert tau[j] == t == 1e-8 * np.mean(np.diag(Sigma[j]))
        St = Sigma[j] + t * np.eye(r)
        cond = np.linalg.cond(St)
        np.testing.assert_allclose(L[j], Lr, rtol=0, atol=1e-14 * cond * np.abs(Lr).max())
        np.testing.assert_allclose(Q[j].dot(St), np.eye(r), rtol=0, atol=1e-13 * cond)
        np.testing.assert_array_equal(Q[j], Q[j].T)
        z = Zp[:, j % m, :]                                            # (S, r)
        np.testing.assert_allclose(F[j], (mu[j] + z.dot(Lr.T)).T, rtol=0, atol=1e-13 * cond * np.abs(F[j]).max())
        Gr = np.linalg.solve(Lr.T, z.T)                                # (r, S)
        np.testing.assert_allclose(G[j], Gr, rtol=0, atol=1e-13 * cond * np.abs(Gr).max())


def test_host_ladder_on_a_rank_deficient_covariance(driver):
    """Two equal pending points: Sigma is singular.  As the device computes it, it carries rounding of the size of the covariance gate
    (1e-8 sigma_f^2): with the duplicated pair's covariance 5e-8 above its variance Sigma is indefinite by -5e-8, rung 0 (1e-8 mean diag)
    fails and rung 1 holds -- the ladder must climb, to NumPy's rung; with one rung allowed the output is reported as j + 1.  The exactly
    singular matrix factorizes on rung 0 (tau makes it definite)."""
    rng = np.random.RandomState(0)
    r, m, S = 4, 2, 3
    pts = rng.uniform(size=(r, 2))
    pts[2] = pts[1]
    d2 = np.sum((pts[:, None, :] - pts[None, :, :]) ** 2, -1)
    exact = np.exp(-0.5 * d2 / 0.3 ** 2)
    assert np.linalg.matrix_rank(exact) == r - 1
    bent = exact.copy()
    bent[1, 2] = bent[2, 1] = exact[1, 1] * (1 + 5e-8)
    Sigma = np.stack([exact, bent])
    mu, Zp = rng.normal(size=(m, r)), rng.normal(size=(S, m, r))
    rc, tau, L, Q, F, G = _run_driver(driver, Sigma, mu, Zp, m, 10)
    assert rc == 0
    rung0 = 1e-8 * np.mean(np.diag(exact))
    assert tau[0] == rung0 == PR.ladder(exact)[0]
    assert tau[1] == PR.ladder(bent)[0] and tau[1] > 5 * rung0, "the indefinite matrix must climb the ladder"
    for j in range(2):
        St = Sigma[j] + tau[j] * np.eye(r)
        np.testing.assert_allclose(L[j].dot(L[j].T), St, rtol=0, atol=1e-14)
        assert np.all(np.isfinite(Q[j])) and np.all(np.isfinite(F[j])) and np.all(np.isfinite(G[j]))
    rc1, tau1, _, _, _, _ = _run_driver(driver, Sigma, mu, Zp, m, 1)
    assert rc1 == 2 and tau1[1] == 1e-8 * np.mean(np.diag(bent))


# ---- surface ---------------------------------------------------------------------------------------------------------------------
def test_header_declares_and_library_exports_the_entry_points():
    header = open(os.path.join(ROOT, "include", "bocf_hip.h")).read()
    lib = _ffi.load()
    for name in ENTRY_POINTS:
        assert re.search(r"\bint %s\(bocf_ctx\* ctx" % name, header), name
        assert name in _ffi.SIGNATURES
        assert isinstance(getattr(lib, name), ctypes._CFuncPtr)
    # argument validation needs no GPU: a null context is refused with the entry point's name
    assert lib.bocf_set_pending_points(None, None, 1, None, 1, 5, None) < 0 and b"bocf_set_pending_points" in lib.bocf_last_error()
    assert lib.bocf_get_pending_samples(None, None) < 0 and b"bocf_get_pending_samples" in lib.bocf_last_error()
    assert lib.bocf_acq_pending(None, 1, None, 0, None, 0, None, 1, None, None) < 0 and b"bocf_acq_pending" in lib.bocf_last_error()


def test_exports_and_model_methods():
    assert B.uEI_pending is B.acquisitions.uEI_pending and issubclass(B.uEI_pending, B.uEI_noiseless)
    assert B.CompositeGreedyBatch is B.cbo.CompositeGreedyBatch
    assert B.uEI_pending.analytical_gradient_prediction is True
    for name in ("set_pending_points", "acq_pending", "pending_samples"):
        assert getattr(B.multi_outputGP, name).__doc__
    from bocf_amd import build
    assert "pending.hip" in build.SOURCES and "capi_pending.hip" in build.SOURCES
    model = B.multi_outputGP(2, fixed_hyps=True)
    assert "pending" in model._resident.__slots__ and model._resident.pending is None
    with pytest.raises(RuntimeError):
        model.set_pending_points(np.zeros((1, 2)), np.zeros((3, 2, 1)))        # no model yet: a clear error
    with pytest.raises(ValueError):
        B.CompositeGreedyBatch(B.uEI_pending.__new__(B.uEI_pending), 17)
    with pytest.raises(TypeError):
        B.CompositeGreedyBatch(object(), 2)


# ---- host logic on a mock device model -------------------------------------------------------------------------------------------
class _MockModel(object):
    analytical_gradient_prediction = True

    def __init__(self, m, d):
        self.output_dim, self._fit_serial, self.calls = m, 1, []

    def number_of_hyps_samples(self):
        return 1

    def _ensure_fitted(self):
        pass

    def acq_linear(self, *a, **kw):
        raise AssertionError("not used")

    def set_pending_points(self, P, Zp, W=None):
        self.calls.append(("pending", np.array(P), np.array(Zp), np.array(W), self._fit_serial))

    def acq_pending(self, X, util_kind, util_params, thetas, prob, W=None, n_hyps=None, grad=False, fetch=True):
        self.calls.append(("acq_pending", util_kind, np.array(thetas), None if prob is None else np.array(prob), np.array(W), grad))
        X = np.atleast_2d(X)
        v = np.sum(X, 1)
        return (v, np.ones(X.shape)) if grad else v

    def acq_mc(self, X, kind, util_kind, util_params, thetas, prob, W=None, fetch=True, n_hyps=None, program=None):
        self.calls.append(("acq_mc", kind, util_kind, np.array(thetas), None if prob is None else np.array(prob), np.array(W)))
        return -np.sum(np.atleast_2d(X), 1)

    def acq_mc_grad(self, X, util_kind, util_params, thetas, prob, W=None, n_hyps=None, program=None):
        self.calls.append(("acq_mc_grad", util_kind, np.array(thetas), None if prob is None else np.array(prob), np.array(W)))
        X = np.atleast_2d(X)
        return -np.sum(X, 1), -np.ones(X.shape)

    def select_topk(self, k):
        return np.arange(k), np.zeros(k)


def _acq(cls, m=3, d=2, seed=11):
    support = np.array([[0.2, 0.3, 0.5], [0.6, 0.1, 0.3]])[:, :m]
    U = B.Utility(parameter_dist=B.ParameterDistribution(support=support, prob_dist=np.array([0.25, 0.75])), device="neg_sq_dist")
    model = _MockModel(m, d)
    np.random.seed(seed)
    return cls(model, None, utility=U), model, support


def test_uei_pending_with_no_pending_points_is_its_parent():
    X = np.random.RandomState(0).uniform(size=(4, 2))
    out = []
    for cls in (B.uEI_noiseless, B.uEI_pending):
        acq, model, _ = _acq(cls)
        if cls is B.uEI_pending:
            acq.set_pending_points(None)
            acq.set_pending_points(np.zeros((0, 2)))
        v = acq._compute_acq(X)
        g = acq._compute_acq_withGradients(X)
        out.append((acq.W_samples, v, g, [c[0] for c in model.calls], [c[1:] for c in model.calls], np.random.uniform()))
    a, b = out
    assert a[3] == b[3] == ["acq_mc", "acq_mc_grad"]
    np.testing.assert_array_equal(a[0], b[0])
    np.testing.assert_array_equal(a[1], b[1])
    np.testing.assert_array_equal(a[2][0], b[2][0])
    np.testing.assert_array_equal(a[2][1], b[2][1])
    assert a[5] == b[5]                                         # the same draws from np.random
    for ca, cb in zip(a[4], b[4]):
        for x, y in zip(ca, cb):
            np.testing.assert_array_equal(x, y)


def test_uei_pending_host_logic():
    acq, model, support = _acq(B.uEI_pending)
    S, m = acq.W_samples.shape
    assert (S, m) == (25, 3) and acq.analytical_gradient_acq
    P = np.array([[0.1, 0.2], [0.3, 0.4]])
    with pytest.raises(ValueError):
        acq.set_pending_points(P, np.zeros((S, m, 3)))
    with pytest.raises(ValueError):
        acq.set_pending_points(np.zeros((16, 2)))
    # Z = None: one np.random.normal(size=(S, m, r))
    state = np.random.get_state()
    acq.set_pending_points(P)
    np.random.set_state(state)
    Z = np.random.normal(size=(S, m, 2))
    np.testing.assert_array_equal(acq.pending_Z, Z)
    X = np.random.RandomState(1).uniform(size=(5, 2))
    v = acq._compute_acq(X)
    assert v.shape == (5, 1) and np.array_equal(v[:, 0], X.sum(1))
    assert [c[0] for c in model.calls] == ["pending", "acq_pending"]
    st, ev = model.calls
    assert np.array_equal(st[1], P) and np.array_equal(st[2], Z) and np.array_equal(st[3], acq.W_samples)
    assert ev[1] == _ffi.UTIL_NEG_SQ_DIST and np.array_equal(ev[2], support) and np.array_equal(ev[3], [0.25, 0.75]) and ev[5] is False
    v, dv = acq._compute_acq_withGradients(X)
    assert dv.shape == (5, 2) and model.calls[-1][5] is True
    f, df = acq.acquisition_function_withGradients(X)
    assert np.array_equal(f, -v) and np.array_equal(df, -dv)
    # a new fit serial: staged again for that fit
    model._fit_serial += 1
    acq._compute_acq(X)
    assert model.calls[-2][0] == "pending" and model.calls[-2][4] == 2
    # a utility without a compiled-in device kind
    dist = B.ParameterDistribution(support=np.array([[0.1, 0.2, 0.3]]), prob_dist=np.array([1.0]))
    U = B.Utility(func=lambda t, y: -np.sum(np.abs(y)), dfunc=lambda t, y: -np.sign(y), parameter_dist=dist)
    odd = B.uEI_pending(_MockModel(3, 2), None, utility=U)
    odd.set_pending_points(P)
    with pytest.raises(NotImplementedError, match="device kind"):
        odd._compute_acq(X)
    with pytest.raises(NotImplementedError, match="device kind"):
        odd._compute_acq_withGradients(X)


class _ScriptedAcq(object):
    """An acquisition whose optimize() returns scripted points and records the pending set in force."""

    def __init__(self, m, d, fail_at=None):
        self.W_samples = np.zeros((7, m))
        self.d, self.log, self.fail_at, self.n = d, [], fail_at, 0
        self.P = self.Z = None

    def set_pending_points(self, P, Z=None):
        self.P, self.Z = (None, None) if P is None else (np.array(P), np.array(Z))
        self.log.append(("set", None if P is None else len(P)))

    def optimize(self, duplicate_manager=None, x_baseline=None):
        if self.n == self.fail_at:
            raise RuntimeError("scripted failure")
        self.log.append(("opt", self.P, self.Z, x_baseline, np.random.uniform()))
        self.n += 1
        return np.full((1, self.d), 0.1 * self.n), -1.0


def test_greedy_batch_draw_order_column_reuse_and_cleanup():
    m, d, q = 3, 2, 4
    acq = _ScriptedAcq(m, d)
    np.random.seed(5)
    X = B.CompositeGreedyBatch(acq, q).compute_batch(x_baseline=np.zeros((1, d)))
    after = np.random.uniform()
    # the draws: optimize 1 (one uniform in the script), ONE normal block (S, m, q - 1), then optimize 2 .. q
    np.random.seed(5)
    u1 = np.random.uniform()
    Z = np.random.normal(size=(7, m, q - 1))
    us = [np.random.uniform() for _ in range(q - 1)]
    assert np.random.uniform() == after
    assert X.shape == (q, d) and np.allclose(X[:, 0], [0.1, 0.2, 0.3, 0.4])
    opts = [e for e in acq.log if e[0] == "opt"]
    assert len(opts) == q and opts[0][1] is None and opts[0][4] == u1
    for k in range(1, q):
        np.testing.assert_array_equal(opts[k][1], X[:k])              # the pending points found so far
        np.testing.assert_array_equal(opts[k][2], Z[:, :, :k])        # the leading k columns of the one draw
        assert opts[k][4] == us[k - 1] and np.array_equal(opts[k][3], np.zeros((1, d)))
    assert acq.log[0] == ("set", None) and acq.log[-1] == ("set", None) and acq.P is None
    # batch_size = 1 is Sequential: no normals drawn
    acq1 = _ScriptedAcq(m, d)
    np.random.seed(5)
    X1 = B.CompositeGreedyBatch(acq1, 1).compute_batch()
    assert X1.shape == (1, d) and np.random.uniform() == np.random.RandomState(5).uniform(size=2)[1]
    # an exception in step 3 leaves no pending points behind
    bad = _ScriptedAcq(m, d, fail_at=2)
    with pytest.raises(RuntimeError, match="scripted"):
        B.CompositeGreedyBatch(bad, q).compute_batch()
    assert bad.P is None and bad.log[-1] == ("set", None)
