"""Look-ahead posterior and discrete composite knowledge gradient on the device (bocf_set_ref_points, bocf_cov_to_ref,
bocf_conditioned_variance, bocf_acq_kg, the multi_outputGP look-ahead methods, uKG) against the NumPy restatement tests/kg_ref.py and
the oracle's own refit with N + 1 points -- never against another device path alone.

Gates: variances and covariances |delta| <= 1e-8 sigma_f^2 + 1e-10; acquisition values rel 1e-5 with an absolute
floor of 1e-12 x the size of the terms KG is a difference of, top-16 index sets equal; gradients rtol 1e-6 / atol 1e-9 scale against the
restatement."""
import ctypes
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import kg_ref as K  # noqa: E402

import bocf_amd as B  # noqa: E402
from bocf_amd import _ffi  # noqa: E402
from oracle import cpu_ref as R  # noqa: E402

pytestmark = pytest.mark.gpu

KERN = {"rbf": B.kern.RBF, "se": B.kern.SE, "matern52": B.kern.Matern52, "matern32": B.kern.Matern32}
KID = {"rbf": _ffi.KERN_RBF, "se": _ffi.KERN_SE, "matern52": _ffi.KERN_MATERN52, "matern32": _ffi.KERN_MATERN32}
UTIL = {"linear": _ffi.UTIL_LINEAR, "neg_sq_dist": _ffi.UTIL_NEG_SQ_DIST, "neg_sum_exp": _ffi.UTIL_NEG_SUM_EXP,
        "neg_exp_cos": _ffi.UTIL_NEG_EXP_COS, "rosenbrock": _ffi.UTIL_ROSENBROCK}
MIXED = ["se", "matern52", "rbf", "matern32"]


def _fixed_model(kinds, X, Y, var, ls, noise):
    d = X.shape[1]
    model = B.multi_outputGP(len(kinds), kernel=[KERN[k](d, variance=var[j], lengthscale=ls[j], ARD=True) for j, k in enumerate(kinds)],
                             noise_var=list(noise), fixed_hyps=True)
    model.updateModel(X, [y[:, None] for y in Y])
    return model


def _hyper_model(kinds, X, Y, var, ls, noise, H):
    """H hyper-samples resident on the device (the state updateModel leaves after learning), hyper-parameters given: sample h scales the
    variances by 1 + 0.1 h and the lengthscales by 1 - 0.05 h.  Returns (model, one LookAhead per hyper-sample)."""
    m = len(kinds)
    model = B.multi_outputGP(m, fixed_hyps=False, n_samples=H)
    model._X, model._Y = np.ascontiguousarray(X), [y[:, None].copy() for y in Y]
    model._kernel_ids = [KID[k] for k in kinds]
    model._instances = [[(var[j] * (1 + 0.1 * h), ls[j] * (1 - 0.05 * h), noise[j]) for j in range(m)] for h in range(H)]
    model._fit()
    las = [K.LookAhead.fit(kinds, X, Y, var * (1 + 0.1 * h), ls * (1 - 0.05 * h), noise) for h in range(H)]
    return model, las


def _gate_var(var):
    return 1e-8 * np.max(var) + 1e-10


# ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("N,na,n", [(200, 1, 5), (200, 7, 300), (500, 130, 129)])
def test_covariance_to_the_reference_set(N, na, n):
    d = 3
    X, Y, var, ls, nz, Xc = K.problem(MIXED, N, d, n, 40 + na, noise=1e-4)
    model = _fixed_model(MIXED, X, Y, var, ls, nz)
    la = K.LookAhead.fit(MIXED, X, Y, var, ls, nz)
    A = np.random.RandomState(na).uniform(size=(na, d))
    want = la.cov(Xc, A)
    model.partial_precomputation_for_covariance(A)
    got = model.posterior_covariance_between_points_partially_precomputed(Xc, A)
    assert got.shape == (4, n, na)
    print("cov_to_ref N %d na %d: max |delta| %.3g (gate %.3g)" % (N, na, np.abs(got - want).max(), _gate_var(var)))
    np.testing.assert_allclose(got, want, rtol=0, atol=_gate_var(var))
    np.testing.assert_allclose(got, model.posterior_covariance_between_points(Xc, A), rtol=0, atol=_gate_var(var))
    with pytest.raises(ValueError):
        model.posterior_covariance_between_points_partially_precomputed(Xc, A + 1e-3)
    # the raw entry point, all outputs, dcov too
    lib, h = _ffi.load(), model._context().handle
    cov, dcov = np.empty((4, n, na)), np.empty((4, n, na, d))
    assert lib.bocf_cov_to_ref(h, -1, _ffi.dptr(cov), _ffi.dptr(dcov)) == 0
    np.testing.assert_array_equal(cov, got)
    ref_d = la.cov_grad(Xc[:40], A)
    scale = np.abs(ref_d).max()
    print("dcov: max |delta| %.3g, scale %.3g" % (np.abs(dcov[:, :40] - ref_d).max(), scale))
    np.testing.assert_allclose(dcov[:, :40], ref_d, rtol=1e-6, atol=1e-9 * scale)


@pytest.mark.parametrize("N", [200, 1024])
def test_conditioned_variance_against_the_refit(N):
    """Variance conditioned on a next point == the oracle's refit on X u {x} (at N = 1024 the refit crosses a 128 padding boundary), a
    different kernel family per output; a next point equal to a training input and query points equal to the next point included.
    noise >= 1e-6: neither fit needs jitter (asserted), so the comparison cannot hide behind it."""
    d = 3
    X, Y, var, ls, nz, Xc = K.problem(MIXED, N, d, 200, 7 + N, noise=1e-6)
    model = _fixed_model(MIXED, X, Y, var, ls, nz)
    assert np.all(np.asarray(model.jitter) == 0)
    for x in (Xc[:1], X[11:12]):
        P = np.concatenate([Xc[1:], x, X[:3]])
        want = np.empty((4, len(P)))
        for j, kind in enumerate(MIXED):
            refit = R.GPFit(kind, np.concatenate([X, x]), np.concatenate([Y[j], [0.1]]).reshape(-1, 1), var[j], ls[j], nz[j])
            assert refit.jitter == 0
            want[j] = refit.raw_posterior_variance(P)[:, 0]
        model.partial_precomputation_for_variance_conditioned_on_next_point(x)
        got = model.posterior_variance_conditioned_on_next_point(P)
        assert got.shape == (4, len(P))
        print("conditioned variance N %d: max |delta| %.3g (gate %.3g)" % (N, np.abs(got - want).max(), _gate_var(var)))
        np.testing.assert_allclose(got, want, rtol=0, atol=_gate_var(var))


def _fd(f, X, h):
    out = []
    for q in range(X.shape[1]):
        Xp, Xm = X.copy(), X.copy()
        Xp[:, q] += h
        Xm[:, q] -= h
        out.append((f(Xp) - f(Xm)) / (2 * h))
    return np.stack(out, -1)


def test_the_three_gradients():
    """posterior_covariance_gradient, its precomputed twin and posterior_variance_gradient_conditioned_on_next_point against the
    restatement (rtol 1e-6, atol 1e-9 scale) and against central differences of the DEVICE values (rtol 1e-4)."""
    d, N, n = 3, 200, 60
    noise = 1e-4
    X, Y, var, ls, nz, Xc = K.problem(MIXED, N, d, n, 3, noise=noise)
    model = _fixed_model(MIXED, X, Y, var, ls, nz)
    la = K.LookAhead.fit(MIXED, X, Y, var, ls, nz)
    x2 = np.random.RandomState(5).uniform(size=(1, d))
    h = 1e-5
    # floor of the differences: device values carry ~ eps sqrt(cond(Ky)) sigma_f^2, cond(Ky) <= (N sigma_f^2 + noise) / noise; / h
    floor = np.finfo(float).eps * np.sqrt((N * var.max() + noise) / noise) * var.max() / h
    want = la.cov_grad(Xc, x2)[:, :, 0, :]
    g1 = model.posterior_covariance_gradient(Xc, x2)
    model.partial_precomputation_for_covariance_gradient(x2)
    g2 = model.posterior_covariance_gradient_partially_precomputed(Xc, x2)
    assert g1.shape == (4, n, d)
    np.testing.assert_array_equal(g1, g2)
    np.testing.assert_allclose(g1, want, rtol=1e-6, atol=1e-9 * np.abs(want).max())
    fd = _fd(lambda P: model.posterior_covariance_between_points(P, x2)[:, :, 0], Xc, h)
    print("cov gradient: vs restatement %.3g, vs device differences %.3g (floor %.3g)" % (np.abs(g1 - want).max(), np.abs(g1 - fd).max(), floor))
    np.testing.assert_allclose(g1, fd, rtol=1e-4, atol=floor)
    model.partial_precomputation_for_variance_conditioned_on_next_point(x2)
    gv = model.posterior_variance_gradient_conditioned_on_next_point(Xc)
    wantv = la.conditioned_variance_grad(Xc, x2)
    assert gv.shape == (4, n, d)
    np.testing.assert_allclose(gv, wantv, rtol=1e-6, atol=1e-9 * np.abs(wantv).max())
    fdv = _fd(model.posterior_variance_conditioned_on_next_point, Xc, h)
    print("conditioned variance gradient: vs restatement %.3g, vs device differences %.3g" % (np.abs(gv - wantv).max(), np.abs(gv - fdv).max()))
    np.testing.assert_allclose(gv, fdv, rtol=1e-4, atol=floor)


# ---------------------------------------------------------------------------------------------------------------------------------
# bocf_acq_kg.  A covering design over the table of the issue: every (mode, utility) the device has, each with L = 1 and with L = 3
# weighted parameters; N in 200 .. 1024, na in {1, 7, 64, 130}, Sf in {1, 16}, H = 1 and hyper_samples = 3 cycle through the cases.
KG_CASES = [
    # mode, utility, L, N, na, Sf, H, seed
    ("mean", "linear", 3, 200, 130, 16, 1, 1), ("mean", "linear", 1, 300, 7, 1, 3, 2),
    ("closed", "neg_sq_dist", 1, 1024, 64, 16, 1, 3), ("closed", "neg_sq_dist", 3, 200, 1, 16, 1, 4),
    ("closed", "neg_sum_exp", 3, 200, 7, 1, 3, 5), ("closed", "neg_sum_exp", 1, 500, 130, 16, 1, 6),
    ("closed", "rosenbrock", 3, 500, 130, 16, 1, 7), ("closed", "rosenbrock", 1, 200, 64, 1, 1, 8),
    ("mc", "linear", 1, 200, 1, 16, 1, 9), ("mc", "linear", 3, 200, 64, 16, 1, 10),
    ("mc", "neg_sq_dist", 3, 200, 64, 1, 3, 11), ("mc", "neg_sq_dist", 1, 300, 7, 16, 1, 12),
    ("mc", "neg_sum_exp", 1, 300, 7, 16, 1, 13), ("mc", "neg_sum_exp", 3, 200, 130, 1, 1, 14),
    ("mc", "neg_exp_cos", 3, 200, 130, 16, 1, 15), ("mc", "neg_exp_cos", 1, 200, 64, 16, 1, 16),
    ("mc", "rosenbrock", 1, 1024, 64, 16, 1, 17), ("mc", "rosenbrock", 3, 200, 7, 16, 3, 18),
]


def _kg_inputs(kind, m, L, na, Sf, d, seed, S=10):
    rng = np.random.RandomState(1000 + seed)
    A = rng.uniform(size=(na, d))
    Zf, W = rng.normal(size=(Sf, m)), rng.normal(size=(S, m))
    if kind == "rosenbrock":
        thetas = rng.uniform(0.2, 1.0, size=(L, 1))
    elif kind in ("neg_sum_exp", "neg_exp_cos"):
        thetas = np.zeros((L, 1))
    else:
        thetas = rng.uniform(-0.5, 0.5, size=(L, m))
    prob = None if L == 1 else rng.dirichlet(np.ones(L))
    params = rng.uniform(0.5, 1.0, size=m) if kind == "neg_exp_cos" else None
    return A, Zf, W, thetas, prob, params


def _ref_kg(las, Xc, A, Zf, thetas, prob, mode, kind, W, params, grad=False):
    rs = [la.kg(Xc, A, Zf, thetas, prob, mode, kind, W, params, grad=grad) for la in las]
    out = dict(kg=np.mean([r["kg"] for r in rs], 0), gap=np.min([r["gap"] for r in rs], 0), vscale=max(r["vscale"] for r in rs))
    if grad:
        out["dkg"] = np.mean([r["dkg"] for r in rs], 0)
    return out


@pytest.mark.parametrize("mode,kind,L,N,na,Sf,H,seed", KG_CASES)
def test_kg_values(mode, kind, L, N, na, Sf, H, seed):
    d, C = 3, 2000
    kinds = MIXED if kind == "rosenbrock" else MIXED[:3]
    m = len(kinds)
    X, Y, var, ls, nz, Xc = K.problem(kinds, N, d, C, seed, noise=1e-4)
    if H == 1:
        model, las = _fixed_model(kinds, X, Y, var, ls, nz), [K.LookAhead.fit(kinds, X, Y, var, ls, nz)]
    else:
        model, las = _hyper_model(kinds, X, Y, var, ls, nz, H)
    A, Zf, W, thetas, prob, params = _kg_inputs(kind, m, L, na, Sf, d, seed)
    ref = _ref_kg(las, Xc, A, Zf, thetas, prob, mode, kind, W, params)
    model.set_reference_points(A)
    kg = model.acq_kg(Xc, mode, UTIL[kind], params, thetas, prob, Zf, W=W)
    assert kg.shape == (C,) and np.all(np.isfinite(kg))
    err = np.abs(kg - ref["kg"])
    print("KG %s %s L %d N %d na %d Sf %d H %d: max |KG| %.3g, negative %.0f %%, max abs err %.3g, max rel err %.3g, term size %.3g"
          % (mode, kind, L, N, na, Sf, H, np.abs(ref["kg"]).max(), 100 * np.mean(ref["kg"] < 0), err.max(),
             np.max(err / np.maximum(np.abs(ref["kg"]), 1e-300)), ref["vscale"]))
    np.testing.assert_allclose(kg, ref["kg"], rtol=1e-5, atol=1e-12 * ref["vscale"])
    # top-16: the device's selection against the restatement's (whose 16th and 17th values must be clearly apart)
    order = np.argsort(-ref["kg"], kind="stable")
    v16, v17 = ref["kg"][order[15]], ref["kg"][order[16]]
    assert v16 - v17 > 1e-4 * abs(v16), "the restatement's 16th and 17th values are too close for this seed: choose another"
    idx, val = model.select_topk(16)
    assert set(idx.tolist()) == set(order[:16].tolist())
    np.testing.assert_array_equal(val, kg[idx])
    # a second identical call is bit-identical; the two halves of the batch equal the whole batch bit for bit
    np.testing.assert_array_equal(model.acq_kg(Xc, mode, UTIL[kind], params, thetas, prob, Zf, W=W), kg)
    half = C // 2 - 37
    np.testing.assert_array_equal(model.acq_kg(Xc[:half], mode, UTIL[kind], params, thetas, prob, Zf, W=W), kg[:half])
    np.testing.assert_array_equal(model.acq_kg(Xc[half:], mode, UTIL[kind], params, thetas, prob, Zf, W=W), kg[half:])


@pytest.mark.parametrize("mode,kind,L,H", [("mean", "linear", 3, 1), ("closed", "neg_sq_dist", 3, 1), ("closed", "neg_sum_exp", 1, 3),
                                           ("closed", "rosenbrock", 3, 1), ("mc", "neg_exp_cos", 3, 1), ("mc", "neg_sq_dist", 1, 3),
                                           ("mc", "rosenbrock", 3, 1)])
def test_kg_gradients(mode, kind, L, H):
    """dKG/dx against the restatement's envelope-rule gradient (rtol 1e-5; floor: the acquisition gate's 1e-12 x the gradient's own
    scale) on candidates with no near tie -- best and second-best inner value of every (fantasy, theta) at least 1e-6 max|KG| apart in
    the restatement; at most 5 % of the candidates may be left out on these grounds."""
    d, N, C, na, Sf = 3, 256, 400, 64, 16
    kinds = MIXED if kind == "rosenbrock" else MIXED[:3]
    m = len(kinds)
    X, Y, var, ls, nz, Xc = K.problem(kinds, N, d, C, 77, noise=1e-4)
    if H == 1:
        model, las = _fixed_model(kinds, X, Y, var, ls, nz), [K.LookAhead.fit(kinds, X, Y, var, ls, nz)]
    else:
        model, las = _hyper_model(kinds, X, Y, var, ls, nz, H)
    A, Zf, W, thetas, prob, params = _kg_inputs(kind, m, L, na, Sf, d, 50)
    ref = _ref_kg(las, Xc, A, Zf, thetas, prob, mode, kind, W, params, grad=True)
    model.set_reference_points(A)
    kg, dkg = model.acq_kg(Xc, mode, UTIL[kind], params, thetas, prob, Zf, W=W, grad=True)
    assert dkg.shape == (C, d)
    np.testing.assert_allclose(kg, ref["kg"], rtol=1e-5, atol=1e-12 * ref["vscale"])
    np.testing.assert_array_equal(kg, model.acq_kg(Xc, mode, UTIL[kind], params, thetas, prob, Zf, W=W))      # the value form computes the same bits
    keep = ref["gap"] >= 1e-6 * np.max(np.abs(ref["kg"]))
    print("KG gradient %s %s: smallest gap %.3g against max |KG| %.3g, %d of %d candidates near-tied, max abs err %.3g, gradient scale %.3g"
          % (mode, kind, ref["gap"].min(), np.abs(ref["kg"]).max(), np.sum(~keep), C, np.abs(dkg[keep] - ref["dkg"][keep]).max(), np.abs(ref["dkg"]).max()))
    assert np.mean(~keep) <= 0.05
    np.testing.assert_allclose(dkg[keep], ref["dkg"][keep], rtol=1e-5, atol=1e-12 * np.abs(ref["dkg"]).max())
    g2 = model.acq_kg(Xc, mode, UTIL[kind], params, thetas, prob, Zf, W=W, grad=True)[1]
    np.testing.assert_array_equal(g2, dkg)


# ---------------------------------------------------------------------------------------------------------------------------------
def test_state_is_left_alone_and_the_reference_set_lifetime():
    d, N, C = 3, 200, 700
    kinds = MIXED[:3]
    X, Y, var, ls, nz, Xc = K.problem(kinds, N, d, C, 5, noise=1e-4)
    model = _fixed_model(kinds, X, Y, var, ls, nz)
    rng = np.random.RandomState(0)
    support, prob = rng.uniform(-0.5, 0.5, size=(2, 3)), np.array([0.4, 0.6])
    U = B.Utility(parameter_dist=B.ParameterDistribution(support=support, prob_dist=prob), device="neg_sq_dist")
    acq = B.uEI_noiseless(model, None, utility=U)
    Zeu = rng.normal(size=(2, 20, 3))
    rows = np.arange(C) % 2

    def snapshot():
        return (model.predict(Xc), acq._compute_acq(Xc), acq._compute_acq_withGradients(Xc[:9]),
                model.expected_utility(Xc, "mc", U, support, rows, Z=Zeu), model.expected_utility(Xc[:9], "closed", U, support, rows[:9], grad=True))
    before = snapshot()
    A, Zf, W, thetas, pr, params = _kg_inputs("neg_sq_dist", 3, 2, 64, 16, d, 3)
    model.set_reference_points(A)
    model.acq_kg(Xc, "closed", _ffi.UTIL_NEG_SQ_DIST, None, thetas, pr, Zf)
    model.acq_kg(Xc[:50], "mean", _ffi.UTIL_LINEAR, None, thetas, pr, Zf, grad=True)
    model.partial_precomputation_for_variance_conditioned_on_next_point(Xc[:1])
    model.posterior_variance_gradient_conditioned_on_next_point(Xc)
    model.posterior_covariance_gradient(Xc, Xc[3:4])
    after = snapshot()

    def same(a, b):
        if a is None:
            assert b is None
        elif isinstance(a, tuple):
            assert len(a) == len(b)
            for x, y in zip(a, b):
                same(x, y)
        else:
            np.testing.assert_array_equal(a, b)
    same(before, after)
    # a KG call does not disturb the uEI acquisition that follows on the same candidates, and the other way round
    lib, h = _ffi.load(), model._context().handle
    model.set_reference_points(A)
    kg = model.acq_kg(Xc, "mc", _ffi.UTIL_NEG_SQ_DIST, None, thetas, pr, Zf, W=acq.W_samples)
    acq._compute_acq(Xc)
    np.testing.assert_array_equal(model.acq_kg(Xc, "mc", _ffi.UTIL_NEG_SQ_DIST, None, thetas, pr, Zf, W=acq.W_samples), kg)
    # a new candidate set keeps the reference set ...
    Xd = _ffi.f64(Xc[:130])
    assert lib.bocf_set_candidates(h, _ffi.dptr(Xd), 130) == 0
    cov = np.empty((3, 130, 64))
    assert lib.bocf_cov_to_ref(h, 0, _ffi.dptr(cov), None) == 0
    np.testing.assert_allclose(cov, K.LookAhead.fit(kinds, X, Y, var, ls, nz).cov(Xd, A), rtol=0, atol=_gate_var(var))
    # ... new targets, an appended observation and a refit drop it, and the next call says so
    for change in ("targets", "append", "refit"):
        model.set_reference_points(A)
        if change == "targets":
            model.updateModel(X, [(y + 0.1)[:, None] for y in Y])
        elif change == "append":
            model.updateModel(np.concatenate([X, Xc[:1]]), [np.concatenate([y, [0.2]])[:, None] for y in Y])
            X, Y = np.concatenate([X, Xc[:1]]), [np.concatenate([y, [0.2]]) for y in Y]
        else:
            model.incremental = False
            model.updateModel(X, [y[:, None] for y in Y])
        model._ensure_fitted()
        assert lib.bocf_set_candidates(h, _ffi.dptr(Xd), 130) == 0
        assert lib.bocf_cov_to_ref(h, 0, _ffi.dptr(cov), None) < 0
        msg = lib.bocf_last_error()
        assert b"bocf_cov_to_ref" in msg and b"no reference points" in msg, (change, msg)
        with pytest.raises(RuntimeError, match="reference points"):
            model.acq_kg(Xd, "mean", _ffi.UTIL_LINEAR, None, thetas, pr, Zf)


def test_every_validation_path_names_its_entry_point():
    d, N = 2, 50
    kinds = MIXED[:3]
    X, Y, var, ls, nz, Xc = K.problem(kinds, N, d, 20, 9, noise=1e-4)
    model = _fixed_model(kinds, X, Y, var, ls, nz)
    lib, h = _ffi.load(), model._context().handle
    dp = _ffi.dptr
    A, Xd = _ffi.f64(Xc[:5]), _ffi.f64(Xc)
    buf = np.empty(3 * 20 * 5 * d)
    th, Zf = _ffi.f64(np.zeros((2, 3))), _ffi.f64(np.zeros((4, 3)))

    def bad(rc, name, text):
        msg = lib.bocf_last_error()
        assert rc < 0 and name.encode() in msg and text.encode() in msg, (rc, msg, text)

    def kg(mode=1, util=_ffi.UTIL_NEG_SQ_DIST, params=None, npar=0, theta=th, tdim=3, L=2, zf=Zf, Sf=4, out=buf):
        return lib.bocf_acq_kg(h, mode, util, dp(params), npar, dp(theta), tdim, None, L, dp(zf), Sf, dp(out), None)
    # before any reference set / candidates
    bad(lib.bocf_cov_to_ref(h, 0, dp(buf), None), "bocf_cov_to_ref", "no reference points")
    bad(lib.bocf_conditioned_variance(h, 0, 0, dp(buf), None), "bocf_conditioned_variance", "no reference points")
    bad(kg(), "bocf_acq_kg", "no reference points")
    bad(lib.bocf_set_ref_points(h, None, 5), "bocf_set_ref_points", "null")
    bad(lib.bocf_set_ref_points(h, dp(A), 0), "bocf_set_ref_points", "na out of range")
    bad(lib.bocf_set_ref_points(h, dp(A), 1025), "bocf_set_ref_points", "na out of range")
    assert lib.bocf_set_ref_points(h, dp(A), 5) == 0
    assert lib.bocf_set_candidates(h, dp(Xd), 0) == 0
    bad(lib.bocf_cov_to_ref(h, 0, dp(buf), None), "bocf_cov_to_ref", "no resident candidates")
    bad(lib.bocf_conditioned_variance(h, 0, 0, dp(buf), None), "bocf_conditioned_variance", "no resident candidates")
    bad(kg(), "bocf_acq_kg", "no resident candidates")
    assert lib.bocf_set_candidates(h, dp(Xd), 20) == 0
    bad(lib.bocf_cov_to_ref(h, 0, None, None), "bocf_cov_to_ref", "null")
    bad(lib.bocf_cov_to_ref(h, 1, dp(buf), None), "bocf_cov_to_ref", "group out of range")
    bad(lib.bocf_conditioned_variance(h, 0, 0, None, None), "bocf_conditioned_variance", "null")
    bad(lib.bocf_conditioned_variance(h, 0, 5, dp(buf), None), "bocf_conditioned_variance", "q out of range")
    bad(lib.bocf_conditioned_variance(h, 0, -1, dp(buf), None), "bocf_conditioned_variance", "q out of range")
    bad(lib.bocf_conditioned_variance(h, 2, 0, dp(buf), None), "bocf_conditioned_variance", "group out of range")
    bad(kg(mode=3), "bocf_acq_kg", "unknown mode")
    bad(kg(util=7), "bocf_acq_kg", "unknown utility kind")
    bad(kg(L=0), "bocf_acq_kg", "L out of range")
    bad(kg(L=33), "bocf_acq_kg", "L out of range")
    bad(kg(theta=None), "bocf_acq_kg", "theta")
    bad(kg(tdim=2), "bocf_acq_kg", "theta_dim must equal m")
    bad(kg(mode=0, util=_ffi.UTIL_NEG_SUM_EXP, tdim=1), "bocf_acq_kg", "theta_dim must equal m")
    bad(kg(util=_ffi.UTIL_ROSENBROCK, tdim=1), "bocf_acq_kg", "even m")
    bad(kg(util=_ffi.UTIL_LINEAR), "bocf_acq_kg", "no closed-form")
    bad(kg(util=_ffi.UTIL_NEG_EXP_COS, tdim=1), "bocf_acq_kg", "no closed-form")
    bad(kg(npar=17, params=np.zeros(17)), "bocf_acq_kg", "utility parameters")
    bad(kg(npar=2), "bocf_acq_kg", "utility parameters")
    bad(kg(zf=None), "bocf_acq_kg", "null Zf")
    bad(kg(Sf=0), "bocf_acq_kg", "Sf out of range")
    bad(kg(Sf=257), "bocf_acq_kg", "Sf out of range")
    bad(kg(mode=2), "bocf_acq_kg", "no Monte-Carlo samples")
    model.set_mc_samples(np.zeros((257, 3)))
    bad(kg(mode=2), "bocf_acq_kg", "more than 256")
    model.set_mc_samples(np.zeros((4, 3)))
    bad(kg(mode=2, util=_ffi.UTIL_NEG_EXP_COS, tdim=1), "bocf_acq_kg", "neg_exp_cos needs m weights")
    assert kg(mode=2) == 0 and kg() == 0
    # the workspace cap: with N = 400 (padded to 512) and 1 MiB not even one chunk of 128 candidates fits (3 x 512 x 128 x 8 bytes)
    X4, Y4, var4, ls4, nz4, _ = K.problem(kinds, 400, d, 1, 10, noise=1e-4)
    big = _fixed_model(kinds, X4, Y4, var4, ls4, nz4)
    hb = big._context().handle
    assert lib.bocf_set_ref_points(hb, dp(A), 5) == 0 and lib.bocf_set_candidates(hb, dp(Xd), 20) == 0
    big.set_option("workspace_mb", 1)
    bad(lib.bocf_acq_kg(hb, 1, _ffi.UTIL_NEG_SQ_DIST, None, 0, dp(th), 3, None, 2, dp(Zf), 4, dp(buf), None), "bocf_acq_kg", "exceeds option workspace_mb")
    bad(lib.bocf_cov_to_ref(hb, 0, dp(buf), None), "bocf_cov_to_ref", "exceeds option workspace_mb")
    bad(lib.bocf_conditioned_variance(hb, 0, 0, dp(buf), None), "bocf_conditioned_variance", "exceeds option workspace_mb")
    bad(lib.bocf_set_ref_points(hb, dp(A), 5), "bocf_set_ref_points", "exceeds option workspace_mb")
    big.set_option("workspace_mb", 24576)
    assert lib.bocf_cov_to_ref(hb, 0, dp(buf), None) == 0
    # the gradient form holds d Sigma / dx of every (output, candidate, reference point): beyond the cap it is refused
    wide = _ffi.f64(np.random.RandomState(2).uniform(size=(1024, d)))
    many = _ffi.f64(np.random.RandomState(3).uniform(size=(60, d)))
    assert lib.bocf_set_ref_points(h, dp(wide), 1024) == 0 and lib.bocf_set_candidates(h, dp(many), 60) == 0
    model.set_option("workspace_mb", 1)
    bigbuf = np.empty(3 * 60 * 1024 * d)
    bad(lib.bocf_acq_kg(h, 1, _ffi.UTIL_NEG_SQ_DIST, None, 0, dp(th), 3, None, 2, dp(Zf), 4, dp(bigbuf), dp(bigbuf)), "bocf_acq_kg", "exceeds option workspace_mb")
    bad(lib.bocf_cov_to_ref(h, 0, dp(bigbuf), dp(bigbuf)), "bocf_cov_to_ref", "exceeds option workspace_mb")
    assert lib.bocf_cov_to_ref(h, 0, dp(bigbuf), None) == 0
    model.set_option("workspace_mb", 24576)
    assert lib.bocf_cov_to_ref(h, 0, dp(bigbuf), dp(bigbuf)) == 0
    assert lib.bocf_set_ref_points(h, dp(A), 5) == 0 and lib.bocf_set_candidates(h, dp(Xd), 20) == 0
    # a host-given posterior has no factor
    canned = _ffi.Context(0)
    mean, vv, mt = np.zeros((1, 4)), np.ones((1, 4)), np.zeros((1, 3))
    _ffi.check(lib.bocf_set_posterior(canned.handle, 1, 4, 3, dp(mean), dp(vv), dp(mt)), "bocf_set_posterior")
    for call, name in ((lambda: lib.bocf_set_ref_points(canned.handle, dp(A), 1), "bocf_set_ref_points"),
                       (lambda: lib.bocf_cov_to_ref(canned.handle, 0, dp(buf), None), "bocf_cov_to_ref"),
                       (lambda: lib.bocf_conditioned_variance(canned.handle, 0, 0, dp(buf), None), "bocf_conditioned_variance"),
                       (lambda: lib.bocf_acq_kg(canned.handle, 0, 0, None, 0, dp(th), 1, None, 1, dp(Zf), 1, dp(buf), None), "bocf_acq_kg")):
        bad(call(), name, "host-given posterior")
    # the context is still usable
    assert lib.bocf_set_ref_points(h, dp(A), 5) == 0 and kg() == 0


# ---------------------------------------------------------------------------------------------------------------------------------
def _bo_problem(seed):
    np.random.seed(seed)
    d, m = 2, 2
    space = B.Design_space([{'name': 'x', 'type': 'continuous', 'domain': (0, 1), 'dimensionality': d}])
    f = [lambda x: np.sin(3 * x[:, :1]) * x[:, 1:2] + x[:, :1] ** 2, lambda x: np.cos(2 * x[:, 1:2]) + 0.5 * x[:, :1]]
    objective = B.MultiObjective(f, noise_var=[1e-4, 1e-4])
    model = B.multi_outputGP(m, kernel=[B.kern.RBF(d, variance=1.0, lengthscale=0.3, ARD=True) for _ in range(m)], noise_var=[1e-4] * m, fixed_hyps=True)
    U = B.Utility(parameter_dist=B.ParameterDistribution(support=np.array([[0.5, 0.2], [0.1, 0.9]]), prob_dist=np.array([0.5, 0.5])), device="neg_sq_dist")
    opt = B.AcquisitionOptimizer(space, optimizer='lbfgs', n_starting=200, n_anchor=6)
    acq = B.uKG(model, space, optimizer=opt, utility=U, n_fantasies=8, n_ref_points=32)
    return space, objective, model, acq, opt, f


def test_ukg_through_the_acquisition_optimizer():
    space, objective, model, acq, opt, f = _bo_problem(31)
    X0 = np.random.uniform(size=(12, 2))
    model.updateModel(X0, [fj(X0) for fj in f])
    x, fx = acq.optimize()
    assert x.shape == (1, 2) and np.all(x >= 0.0) and np.all(x <= 1.0)
    best_anchor = np.max(-opt.last_info["anchor_points_values"])
    value = acq._compute_acq(x)[0, 0]
    assert value == -float(np.squeeze(fx))
    print("uKG optimum %.6g against its best anchor %.6g" % (value, best_anchor))
    assert value >= best_anchor
    assert acq.reference_points.shape == (32, 2) and any(np.array_equal(acq.reference_points[-1], r) for r in X0)
    # against the restatement at the optimum and the anchors
    la = K.LookAhead.fit(["rbf", "rbf"], X0, [fj(X0)[:, 0] for fj in f], [1.0, 1.0], [np.full(2, 0.3)] * 2, [1e-4, 1e-4])
    P = np.concatenate([x, opt.last_info["anchor_points"]])
    ref = la.kg(P, acq.reference_points, acq.Z_samples, acq.utility.parameter_dist.support, acq.utility_prob_dist, "closed", "neg_sq_dist")
    np.testing.assert_allclose(acq._compute_acq(P)[:, 0], ref["kg"], rtol=1e-5, atol=1e-12 * ref["vscale"])
    assert len(acq.select_anchors(4)) == 4


def test_one_cbo_iteration_with_sequential_ukg():
    space, objective, model, acq, opt, f = _bo_problem(32)
    X0 = np.random.uniform(size=(6, 2))
    bo = B.CBO(model, space, objective, acq, B.Sequential(acq), X0)
    bo.run_optimization(max_iter=1)
    assert bo.X.shape == (7, 2) and np.all(bo.X >= 0.0) and np.all(bo.X <= 1.0)
    assert [y.shape for y in bo.Y] == [(7, 1), (7, 1)]


def test_full_size_property_run():
    """N = 1024, d = 6, m = 4, C = 8192, na = 128, Sf = 32, closed form: finite, reproducible bit for bit, and the top-16 equal the
    restatement's on a 512-candidate subsample that contains them."""
    N, d, C, na, Sf = 1024, 6, 8192, 128, 32
    X, Y, var, ls, nz, Xc = K.problem(MIXED, N, d, C, 123, noise=1e-4)
    model = _fixed_model(MIXED, X, Y, var, ls, nz)
    A, Zf, W, thetas, prob, params = _kg_inputs("neg_sq_dist", 4, 3, na, Sf, d, 99)
    model.set_reference_points(A)
    kg = model.acq_kg(Xc, "closed", _ffi.UTIL_NEG_SQ_DIST, None, thetas, prob, Zf)
    assert kg.shape == (C,) and np.all(np.isfinite(kg))
    idx, val = model.select_topk(16)
    np.testing.assert_array_equal(model.acq_kg(Xc, "closed", _ffi.UTIL_NEG_SQ_DIST, None, thetas, prob, Zf), kg)
    rest = np.setdiff1d(np.arange(C), idx)
    sub = np.concatenate([idx, np.random.RandomState(1).choice(rest, 512 - 16, replace=False)])
    ref = K.LookAhead.fit(MIXED, X, Y, var, ls, nz).kg(Xc[sub], A, Zf, thetas, prob, "closed", "neg_sq_dist")
    np.testing.assert_allclose(kg[sub], ref["kg"], rtol=1e-5, atol=1e-12 * ref["vscale"])
    order = np.argsort(-ref["kg"], kind="stable")
    assert ref["kg"][order[15]] - ref["kg"][order[16]] > 1e-4 * abs(ref["kg"][order[15]]), "16th and 17th too close for this seed: choose another"
    assert set(sub[order[:16]].tolist()) == set(idx.tolist())
