"""Greedy q-point batches on the device: the Monte-Carlo expected improvement of the composite utility conditioned on pending points
(bocf_set_pending_points, bocf_get_pending_samples, bocf_acq_pending, multi_outputGP.set_pending_points / acq_pending, uEI_pending,
CompositeGreedyBatch) against the NumPy restatement tests/pending_ref.py (its bordered-Cholesky route) -- never against another device
path alone.

Gates: values rtol 1e-5 with an absolute floor of 1e-12 x the largest |U| met (the gate of test_gpu_kg.test_kg_values: this path shares
the knowledge gradient's inputs); gradients rtol 1e-5 / atol 1e-12 max|gradient| on the candidates with no sample within 1e-6 scale of its
threshold.  The seeds of the cases are checked on the CPU (tests/test_pending_cpu.py)."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import kg_ref as K  # noqa: E402
import pending_ref as PR  # noqa: E402

import bocf_amd as B  # noqa: E402
from bocf_amd import _ffi  # noqa: E402

pytestmark = pytest.mark.gpu

KERN = {"rbf": B.kern.RBF, "se": B.kern.SE, "matern52": B.kern.Matern52, "matern32": B.kern.Matern32}
KID = {"rbf": _ffi.KERN_RBF, "se": _ffi.KERN_SE, "matern52": _ffi.KERN_MATERN52, "matern32": _ffi.KERN_MATERN32}
UTIL = {"linear": _ffi.UTIL_LINEAR, "neg_sq_dist": _ffi.UTIL_NEG_SQ_DIST, "neg_sum_exp": _ffi.UTIL_NEG_SUM_EXP,
        "neg_exp_cos": _ffi.UTIL_NEG_EXP_COS, "rosenbrock": _ffi.UTIL_ROSENBROCK}
IDS = ["N%d-d%d-m%d-r%d-S%d-L%d-H%d-C%d-%s" % c[:9] for c in PR.CASES]
NGRAD = 40          # candidates of a case the gradient test uses


def _fixed_model(kinds, X, Y, var, ls, noise):
    d = X.shape[1]
    model = B.multi_outputGP(len(kinds), kernel=[KERN[k](d, variance=var[j], lengthscale=ls[j], ARD=True) for j, k in enumerate(kinds)],
                             noise_var=list(noise), fixed_hyps=True)
    model.updateModel(X, [y[:, None] for y in Y])
    return model


def _hyper_model(kinds, X, Y, var, ls, noise, H):
    """H hyper-samples resident on the device, hyper-parameters given as pending_ref.case_lookaheads scales them."""
    m = len(kinds)
    model = B.multi_outputGP(m, fixed_hyps=False, n_samples=H)
    model._X, model._Y = np.ascontiguousarray(X), [y[:, None].copy() for y in Y]
    model._kernel_ids = [KID[k] for k in kinds]
    model._instances = [[(var[j] * (1 + 0.1 * h), ls[j] * (1 - 0.05 * h), noise[j]) for j in range(m)] for h in range(H)]
    model._fit()
    return model


_CACHE = {}


def _case(case):
    """(inputs, device model, restatement of all candidates, restatement with gradients of the first NGRAD) of a case, made once."""
    if case not in _CACHE:
        inp = PR.case_inputs(*case)
        las = PR.case_lookaheads(inp)
        a = (inp["kinds"], inp["X"], inp["Y"], inp["var"], inp["ls"], inp["nz"])
        model = _fixed_model(*a) if inp["H"] == 1 else _hyper_model(*a, inp["H"])
        _CACHE.clear()                                    # one case's model and references at a time
        _CACHE[case] = (inp, model, PR.case_reference(inp, las), PR.case_reference(inp, las, grad=True, n=NGRAD))
    return _CACHE[case]


def _device(model, inp, X, grad=False):
    model.set_hyperparameters(0)              # the best-so-far is that of the hyper-sample current on entry; a call leaves the model on the last
    model.set_pending_points(inp["P"], inp["Zp"], W=inp["W"])
    return model.acq_pending(X, UTIL[inp["kind"]], inp["params"], inp["thetas"], inp["prob"], W=inp["W"], grad=grad)


# ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", PR.CASES, ids=IDS)
def test_values_against_the_restatement(case):
    inp, model, ref, _ = _case(case)
    Xc, C = inp["Xc"], case[7]
    got = _device(model, inp, Xc)
    assert got.shape == (C,) and np.all(np.isfinite(got)) and np.all(got >= 0)
    err = np.abs(got - ref["alpha"])
    print("pending %s: max alpha %.3g, share > 0 %.2f, max abs err %.3g, max rel err %.3g, scale %.3g, jitter %.3g"
          % (IDS[PR.CASES.index(case)], ref["alpha"].max(), np.mean(ref["alpha"] > 0), err.max(),
             np.max(err / np.maximum(np.abs(ref["alpha"]), 1e-300) * (ref["alpha"] > 0)), ref["scale"], model.last_pending_jitter.max()))
    np.testing.assert_allclose(model.last_pending_jitter, ref["tau"], rtol=1e-6)          # rung 0 on both sides
    np.testing.assert_allclose(got, ref["alpha"], rtol=1e-5, atol=1e-12 * ref["scale"])
    # the joint samples at the pending points: F = mu + L z, L from the device's Sigma(P, P) (gate 1e-8 sigma_f^2 + 1e-10 per entry, r entries
    # per row); a perturbation dSigma moves L by at most ~ cond(Sigma~) |dSigma| / |L| -- |L| ~ 1 here
    F = model.pending_samples().transpose(2, 0, 1)                       # (S, M, r)
    atol_F = ref["cond"] * (1e-8 * 1.6 * 1.2 + 1e-10) * case[3] * np.abs(inp["Zp"]).max() + 1e-7
    print("   samples at the pending points: max abs err %.3g (bound %.3g)" % (np.abs(F - ref["F"]).max(), atol_F))
    np.testing.assert_allclose(F, ref["F"], rtol=1e-6, atol=atol_F)
    # a second identical call is bit-identical; the two halves of the batch equal the whole batch bit for bit
    np.testing.assert_array_equal(_device(model, inp, Xc), got)
    if C > 1:
        half = C // 2
        np.testing.assert_array_equal(_device(model, inp, Xc[:half]), got[:half])
        np.testing.assert_array_equal(_device(model, inp, Xc[half:]), got[half:])
    # the values stay on the device for the selection
    k = min(4, C)
    idx, val = model.select_topk(k)
    np.testing.assert_array_equal(val, np.sort(got[half:] if C > 1 else got)[::-1][:k])


@pytest.mark.parametrize("case", PR.CASES, ids=IDS)
def test_gradients_against_the_restatement(case):
    inp, model, _, ref = _case(case)
    X = inp["Xc"][:NGRAD]
    got, dgot = _device(model, inp, X, grad=True)
    assert dgot.shape == X.shape
    np.testing.assert_allclose(got, ref["alpha"], rtol=1e-5, atol=1e-12 * ref["scale"])
    np.testing.assert_array_equal(got, _device(model, inp, X))           # the value form computes the same bits
    keep = ref["gap"] >= 1e-6 * ref["scale"]
    gscale = np.abs(ref["dalpha"]).max()
    print("pending gradient %s: %d of %d candidates near a threshold, %d with a nonzero gradient, max abs err %.3g, gradient scale %.3g"
          % (IDS[PR.CASES.index(case)], np.sum(~keep), len(X), np.sum(np.any(ref["dalpha"] != 0, 1)),
             np.abs(dgot[keep] - ref["dalpha"][keep]).max() if keep.any() else 0.0, gscale))
    assert np.mean(~keep) <= 0.05
    np.testing.assert_allclose(dgot[keep], ref["dalpha"][keep], rtol=1e-5, atol=1e-12 * gscale)
    np.testing.assert_array_equal(_device(model, inp, X, grad=True)[1], dgot)


def test_leading_columns_of_the_normals_give_the_same_samples():
    """The same P at r = 7 with Zp's leading 3 columns gives the F of the r = 3 call for those points: L's leading block depends on the
    leading block of Sigma~ only.  Sigma~ carries the jitter tau = 1e-8 mean diag, taken over 7 or over 3 points: the two factors differ
    by that (to first order |dL| <= |L| |dtau| / lambda_min(Sigma~)), nothing else."""
    case = PR.CASES[[c[:9] for c in PR.CASES].index(PR.SHAPES[1] + ("neg_sq_dist",))]
    inp, model, ref, _ = _case(case)
    model.set_pending_points(inp["P"], inp["Zp"], W=inp["W"])
    F7, tau7 = model.pending_samples(), model.last_pending_jitter.copy()
    model.set_pending_points(inp["P"][:3], np.ascontiguousarray(inp["Zp"][:, :, :3]), W=inp["W"])
    F3, tau3 = model.pending_samples(), model.last_pending_jitter.copy()
    assert F7.shape == (4, 7, 64) and F3.shape == (4, 3, 64)
    st = PR.pending_state(PR.case_lookaheads(inp)[0], inp["P"][:3], inp["Zp"][:, :, :3])
    ev = [np.linalg.eigvalsh(0.5 * (st["Sigma"][j] + st["Sigma"][j].T) + st["tau"][j] * np.eye(3)) for j in range(4)]
    bound = 2 * np.abs(tau7 - tau3).max() * max(np.sqrt(e[-1]) / e[0] for e in ev) * 3 * np.abs(inp["Zp"]).max()
    print("leading block: max |F7 - F3| %.3g (bound %.3g)" % (np.abs(F7[:, :3] - F3).max(), bound))
    np.testing.assert_allclose(F7[:, :3], F3, rtol=0, atol=bound)
    np.testing.assert_allclose(F7[:, :3], ref["F"].transpose(1, 2, 0)[:, :3], rtol=1e-6, atol=1e-6)


def test_state_is_left_alone_and_the_pending_set_lifetime():
    d, N, C = 3, 200, 300
    kinds = PR.MIXED[:3]
    X, Y, var, ls, nz, Xc = K.problem(kinds, N, d, C, 5, noise=1e-4)
    model = _fixed_model(kinds, X, Y, var, ls, nz)
    rng = np.random.RandomState(0)
    support, prob = rng.uniform(-0.5, 0.5, size=(2, 3)), np.array([0.4, 0.6])
    U = B.Utility(parameter_dist=B.ParameterDistribution(support=support, prob_dist=prob), device="neg_sq_dist")
    acq = B.uEI_noiseless(model, None, utility=U)
    W = acq.W_samples
    A, Zf = rng.uniform(size=(9, d)), rng.normal(size=(4, 3))
    lib, h = _ffi.load(), model._context().handle

    def snapshot():
        model.set_reference_points(A)
        kg = model.acq_kg(Xc, "closed", _ffi.UTIL_NEG_SQ_DIST, None, support, prob, Zf)
        cov = np.empty((3, C, 9))
        assert lib.bocf_cov_to_ref(h, 0, _ffi.dptr(cov), None) == 0
        return (kg, cov, model.predict(Xc), acq._compute_acq(Xc), acq._compute_acq_withGradients(Xc[:9]))
    before = snapshot()
    ref_key = model._resident.reference
    P, Zp = rng.uniform(size=(5, d)), rng.normal(size=(25, 3, 5))
    model.set_pending_points(P, Zp, W=W)
    a1 = model.acq_pending(Xc, _ffi.UTIL_NEG_SQ_DIST, None, support, prob, W=W)
    model.acq_pending(Xc[:20], _ffi.UTIL_NEG_SQ_DIST, None, support, prob, W=W, grad=True)
    # the reference set survived: cov_to_ref answers without staging it again, with the same bits
    assert model._resident.reference == ref_key
    assert lib.bocf_set_candidates(h, _ffi.dptr(_ffi.f64(Xc)), C) == 0
    cov = np.empty((3, C, 9))
    assert lib.bocf_cov_to_ref(h, 0, _ffi.dptr(cov), None) == 0
    np.testing.assert_array_equal(cov, before[1])
    # the uEI acquisition right behind a pending call (the best-so-far cache and W are as they were), then everything else
    np.testing.assert_array_equal(acq._compute_acq(Xc), before[3])
    after = snapshot()
    for x, y in zip(before, after):
        for u, v in zip(x if isinstance(x, tuple) else (x,), y if isinstance(y, tuple) else (y,)):
            np.testing.assert_array_equal(u, v)
    # ... and the other way round: the pending values after all of that
    np.testing.assert_array_equal(model.acq_pending(Xc, _ffi.UTIL_NEG_SQ_DIST, None, support, prob, W=W), a1)
    # new targets, an appended observation and a refit drop the pending set, and the next call says so
    out = np.empty(C)
    th = _ffi.f64(support)
    for change in ("targets", "append", "refit"):
        model.set_pending_points(P, Zp, W=W)
        if change == "targets":
            model.updateModel(X, [(y + 0.1)[:, None] for y in Y])
        elif change == "append":
            model.updateModel(np.concatenate([X, Xc[:1]]), [np.concatenate([y, [0.2]])[:, None] for y in Y])
            X, Y = np.concatenate([X, Xc[:1]]), [np.concatenate([y, [0.2]]) for y in Y]
        else:
            model.incremental = False
            model.updateModel(X, [y[:, None] for y in Y])
        model._ensure_fitted()
        model.set_mc_samples(W)
        assert lib.bocf_set_candidates(h, _ffi.dptr(_ffi.f64(Xc)), C) == 0
        assert lib.bocf_acq_pending(h, _ffi.UTIL_NEG_SQ_DIST, None, 0, _ffi.dptr(th), 3, None, 2, _ffi.dptr(out), None) < 0
        msg = lib.bocf_last_error()
        assert b"bocf_acq_pending" in msg and b"no pending points" in msg, (change, msg)
        with pytest.raises(RuntimeError, match="pending points"):
            model.acq_pending(Xc, _ffi.UTIL_NEG_SQ_DIST, None, support, prob, W=W)


def test_every_validation_path_names_its_entry_point():
    d, N = 2, 50
    kinds = PR.MIXED[:3]
    X, Y, var, ls, nz, Xc = K.problem(kinds, N, d, 300, 9, noise=1e-4)
    model = _fixed_model(kinds, X, Y, var, ls, nz)
    model._ensure_fitted()
    lib, h = _ffi.load(), model._context().handle
    dp = _ffi.dptr
    P, Xd = _ffi.f64(Xc[:16]), _ffi.f64(Xc[:20])
    S = 4
    Zp, th, out = _ffi.f64(np.random.RandomState(1).normal(size=(S, 3, 16))), _ffi.f64(np.zeros((2, 3))), np.empty(300 * d)
    jit = np.empty(3)

    def bad(rc, name, text):
        msg = lib.bocf_last_error()
        assert rc < 0 and name.encode() in msg and text.encode() in msg, (rc, msg, text)

    def stage(xp=P, r=5, zp=Zp, s=S, tries=5):
        return lib.bocf_set_pending_points(h, dp(xp), r, dp(zp), s, tries, dp(jit))

    def acq(util=_ffi.UTIL_NEG_SQ_DIST, params=None, npar=0, theta=th, tdim=3, L=2, o=out, g=None):
        return lib.bocf_acq_pending(h, util, dp(params), npar, dp(theta), tdim, None, L, dp(o), dp(g))
    assert lib.bocf_set_candidates(h, dp(Xd), 20) == 0
    bad(stage(), "bocf_set_pending_points", "no Monte-Carlo samples")
    bad(acq(), "bocf_acq_pending", "no Monte-Carlo samples")
    model.set_mc_samples(np.random.RandomState(2).normal(size=(S, 3)))
    bad(acq(), "bocf_acq_pending", "no pending points")
    bad(lib.bocf_get_pending_samples(h, dp(out)), "bocf_get_pending_samples", "no pending points")
    bad(stage(xp=None), "bocf_set_pending_points", "null Xp")
    bad(stage(r=0), "bocf_set_pending_points", "r out of range")
    bad(stage(r=16), "bocf_set_pending_points", "r out of range")
    bad(stage(zp=None), "bocf_set_pending_points", "null Zp")
    bad(stage(s=0), "bocf_set_pending_points", "S out of range")
    bad(stage(s=257), "bocf_set_pending_points", "S out of range")
    bad(stage(s=S + 1), "bocf_set_pending_points", "S must equal")
    assert stage() == 0 and np.all(jit > 0)
    bad(lib.bocf_get_pending_samples(h, None), "bocf_get_pending_samples", "null")
    assert lib.bocf_set_candidates(h, dp(Xd), 0) == 0
    bad(acq(), "bocf_acq_pending", "no resident candidates")
    assert lib.bocf_set_candidates(h, dp(Xd), 20) == 0
    bad(acq(util=_ffi.UTIL_PROGRAM), "bocf_acq_pending", "BOCF_UTIL_PROGRAM")
    bad(acq(util=7), "bocf_acq_pending", "unknown utility kind")
    bad(acq(util=-1), "bocf_acq_pending", "unknown utility kind")
    bad(acq(L=0), "bocf_acq_pending", "L out of range")
    bad(acq(L=33), "bocf_acq_pending", "L out of range")
    bad(acq(theta=None), "bocf_acq_pending", "theta")
    bad(acq(tdim=2), "bocf_acq_pending", "theta_dim must equal m")
    bad(acq(util=_ffi.UTIL_ROSENBROCK, tdim=1), "bocf_acq_pending", "even m")
    bad(acq(npar=17, params=np.zeros(17)), "bocf_acq_pending", "utility parameters")
    bad(acq(npar=2), "bocf_acq_pending", "utility parameters")
    bad(acq(util=_ffi.UTIL_NEG_EXP_COS, tdim=1), "bocf_acq_pending", "neg_exp_cos needs m weights")
    model.set_mc_samples(np.zeros((S + 1, 3)))
    bad(acq(), "bocf_acq_pending", "changed since bocf_set_pending_points")
    model.set_mc_samples(np.random.RandomState(2).normal(size=(S, 3)))
    assert acq() == 0 and acq(g=np.empty(20 * d)) == 0
    # the gradient form is one chunk: with 1 MiB the chunk is 256 candidates (3 x 128 x 8 bytes per column), 300 do not fit; the value form
    # works them off in two chunks
    big = _ffi.f64(Xc)
    assert lib.bocf_set_candidates(h, dp(big), 300) == 0
    whole = np.empty(300)
    assert acq(o=whole) == 0
    model.set_option("workspace_mb", 1)
    chunked = np.empty(300)
    assert acq(o=chunked) == 0
    np.testing.assert_array_equal(chunked, whole)
    bad(acq(g=np.empty(300 * d)), "bocf_acq_pending", "exceeds option workspace_mb")
    model.set_option("workspace_mb", 24576)
    # with N = 400 (padded to 512) and 1 MiB neither the staging (2 x 3 x 512 x 128 x 8 bytes) nor one chunk of 128 candidates fits
    X4, Y4, var4, ls4, nz4, _ = K.problem(kinds, 400, d, 1, 10, noise=1e-4)
    bigm = _fixed_model(kinds, X4, Y4, var4, ls4, nz4)
    bigm.set_mc_samples(np.zeros((S, 3)))
    hb = bigm._context().handle
    assert lib.bocf_set_candidates(hb, dp(Xd), 20) == 0
    assert lib.bocf_set_pending_points(hb, dp(P), 5, dp(Zp), S, 5, None) == 0
    bigm.set_option("workspace_mb", 1)
    bad(lib.bocf_acq_pending(hb, _ffi.UTIL_NEG_SQ_DIST, None, 0, dp(th), 3, None, 2, dp(out), None), "bocf_acq_pending", "exceeds option workspace_mb")
    bad(lib.bocf_set_pending_points(hb, dp(P), 5, dp(Zp), S, 5, None), "bocf_set_pending_points", "exceeds option workspace_mb")
    bigm.set_option("workspace_mb", 24576)
    # a host-given posterior has no factor
    canned = _ffi.Context(0)
    mean, vv, mt = np.zeros((1, 4)), np.ones((1, 4)), np.zeros((1, 3))
    _ffi.check(lib.bocf_set_posterior(canned.handle, 1, 4, 3, dp(mean), dp(vv), dp(mt)), "bocf_set_posterior")
    bad(lib.bocf_set_pending_points(canned.handle, dp(P), 1, dp(Zp), S, 5, None), "bocf_set_pending_points", "host-given posterior")
    bad(lib.bocf_acq_pending(canned.handle, 1, None, 0, dp(th), 1, None, 1, dp(out), None), "bocf_acq_pending", "host-given posterior")
    bad(lib.bocf_get_pending_samples(canned.handle, dp(out)), "bocf_get_pending_samples", "host-given posterior")
    # two equal pending points with one rung allowed: reported per output (j + 1) when Sigma stays indefinite, else staged; either way
    # the context is still usable
    twice = _ffi.f64(np.concatenate([Xc[:1], Xc[:1], Xc[2:4]]))
    rc = lib.bocf_set_pending_points(h, dp(twice), 4, dp(_ffi.f64(Zp[:, :, :4])), S, 10, dp(jit))
    assert rc == 0 and np.all(jit > 0), (rc, lib.bocf_last_error())
    assert lib.bocf_set_candidates(h, dp(Xd), 20) == 0 and acq() == 0 and np.all(np.isfinite(out[:20]))
    assert stage() == 0 and acq() == 0


# ---------------------------------------------------------------------------------------------------------------------------------
def _bo_problem(seed, cls=B.uEI_pending):
    np.random.seed(seed)
    d, m = 2, 2
    space = B.Design_space([{'name': 'x', 'type': 'continuous', 'domain': (0, 1), 'dimensionality': d}])
    f = [lambda x: np.sin(3 * x[:, :1]) * x[:, 1:2] + x[:, :1] ** 2, lambda x: np.cos(2 * x[:, 1:2]) + 0.5 * x[:, :1]]
    objective = B.MultiObjective(f, noise_var=[1e-4, 1e-4])
    model = B.multi_outputGP(m, kernel=[B.kern.RBF(d, variance=1.0, lengthscale=0.3, ARD=True) for _ in range(m)], noise_var=[1e-4] * m, fixed_hyps=True)
    U = B.Utility(parameter_dist=B.ParameterDistribution(support=np.array([[0.5, 0.2], [0.1, 0.9]]), prob_dist=np.array([0.5, 0.5])), device="neg_sq_dist")
    opt = B.AcquisitionOptimizer(space, optimizer='lbfgs', n_starting=200, n_anchor=6)
    acq = cls(model, space, optimizer=opt, utility=U)
    return space, objective, model, acq, opt, f


def test_uei_pending_through_the_acquisition_optimizer():
    space, objective, model, acq, opt, f = _bo_problem(31)
    X0 = np.random.uniform(size=(12, 2))
    model.updateModel(X0, [fj(X0) for fj in f])
    x1, _ = acq.optimize()
    P = np.concatenate([x1, np.random.uniform(size=(1, 2))])
    acq.set_pending_points(P)
    x, fx = acq.optimize()
    assert x.shape == (1, 2) and np.all(x >= 0.0) and np.all(x <= 1.0)
    value = acq._compute_acq(x)[0, 0]
    assert value == -float(np.squeeze(fx))
    best_anchor = np.max(-opt.last_info["anchor_points_values"])
    print("uEI_pending optimum %.6g against its best anchor %.6g" % (value, best_anchor))
    assert value >= best_anchor and value > 0
    # against the restatement at the optimum and the anchors
    la = K.LookAhead.fit(["rbf", "rbf"], X0, [fj(X0)[:, 0] for fj in f], [1.0, 1.0], [np.full(2, 0.3)] * 2, [1e-4, 1e-4])
    Q = np.concatenate([x, opt.last_info["anchor_points"]])
    ref = PR.pending(la, Q, P, acq.pending_Z, acq.W_samples, acq.utility.parameter_dist.support, acq.utility_prob_dist, "neg_sq_dist")
    np.testing.assert_allclose(acq._compute_acq(Q)[:, 0], ref["alpha"], rtol=1e-5, atol=1e-12 * ref["scale"])
    # no pending points: the parent, bit for bit
    acq.set_pending_points(None)
    parent = B.uEI_noiseless(model, space, optimizer=opt, utility=acq.utility)
    parent.W_samples = acq.W_samples
    np.testing.assert_array_equal(acq._compute_acq(Q), parent._compute_acq(Q))


def test_one_cbo_iteration_with_a_greedy_batch():
    space, objective, model, acq, opt, f = _bo_problem(32)
    X0 = np.random.uniform(size=(6, 2))
    state = np.random.get_state()
    bo = B.CBO(model, space, objective, acq, B.CompositeGreedyBatch(acq, 4), X0)
    bo.run_optimization(max_iter=1)
    assert bo.X.shape == (10, 2) and np.all(bo.X >= 0.0) and np.all(bo.X <= 1.0)
    assert [y.shape for y in bo.Y] == [(10, 1), (10, 1)]
    assert acq.pending_points is None
    assert len(np.unique(bo.X[6:], axis=0)) == 4
    # point 1 equals Sequential's under the same seed
    space2, objective2, model2, acq2, opt2, f2 = _bo_problem(32, B.uEI_noiseless)
    np.random.set_state(state)
    bo2 = B.CBO(model2, space2, objective2, acq2, B.Sequential(acq2), X0)
    bo2.run_optimization(max_iter=1)
    np.testing.assert_array_equal(bo2.X[6], bo.X[6])
