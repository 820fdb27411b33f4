"""Joint q-point expected improvement of the composite utility on the device (bocf_acq_joint, multi_outputGP.acq_joint, uEI_joint,
CompositeJointBatch) against the NumPy restatement tests/joint_ref.py on the oracle -- never against another device path alone.

Gates: those of tests/test_gpu_pending.py, which shares every upstream quantity (mean, V, Sigma, their gradients): values rtol 1e-5 with
an absolute floor of 1e-12 x the largest |U| met; gradients rtol 1e-5 / atol 1e-12 max|gradient| on the batches whose smallest margin to
a kink (over (l, s): the gap between the best and the second-best point, and |u - best|) is above 1e-6 x scale.  Caps asserted on the
restatement before the device is looked at: the kink filter drops at most 1/8 of a case's batches, cond(Sigma_j + tau_j I) <= 1e4, and
alpha > 1e-6 x scale on at least 3/4 of the batches (tests/test_joint_cpu.py checks the same caps where a seed can be changed)."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import joint_ref as J  # noqa: E402
import kg_ref as K  # noqa: E402
import pending_ref as PR  # noqa: E402

import bocf_amd as B  # noqa: E402
from bocf_amd import _ffi  # noqa: E402

pytestmark = pytest.mark.gpu

KERN = {"rbf": B.kern.RBF, "se": B.kern.SE, "matern52": B.kern.Matern52, "matern32": B.kern.Matern32}
KID = {"rbf": _ffi.KERN_RBF, "se": _ffi.KERN_SE, "matern52": _ffi.KERN_MATERN52, "matern32": _ffi.KERN_MATERN32}
UTIL = {"linear": _ffi.UTIL_LINEAR, "neg_sq_dist": _ffi.UTIL_NEG_SQ_DIST, "neg_sum_exp": _ffi.UTIL_NEG_SUM_EXP,
        "neg_exp_cos": _ffi.UTIL_NEG_EXP_COS, "rosenbrock": _ffi.UTIL_ROSENBROCK}


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


def _case(case, grad=True):
    """(inputs, device model, restatement, incumbents) of a case, made once; the caps hold before the device computes anything."""
    if case not in _CACHE:
        inp = J.case_inputs(*case)
        las = PR.case_lookaheads(inp)
        ref, best = J.case_reference(inp, las, grad=grad)
        nb = len(ref["alpha"])
        assert ref["cond"] <= 1e4
        assert np.sum(ref["margin"] <= 1e-6 * ref["scale"]) <= nb / 8.0
        assert np.sum(ref["alpha"] > 1e-6 * ref["scale"]) >= 0.75 * nb
        a = (inp["kinds"], inp["X"], inp["Y"], inp["var"], inp["ls"], inp["nz"])
        model = _fixed_model(*a) if inp["H"] == 1 else _hyper_model(*a, inp["H"])
        _CACHE.clear()                                    # one case's model and references at a time
        _CACHE[case] = (inp, model, ref, best)
    return _CACHE[case]


def _device(model, inp, Xb, best, grad=False):
    model.set_hyperparameters(0)              # the default incumbent is that of the hyper-sample current on entry; a call leaves the model on the last
    return model.acq_joint(Xb, inp["q"], UTIL[inp["kind"]], inp["params"], inp["thetas"], inp["prob"], inp["Z"], best=best, grad=grad)


# ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", J.CASES, ids=[J.case_id(c) for c in J.CASES])
def test_values_and_gradients_against_the_restatement(case):
    inp, model, ref, best = _case(case)
    Xb = inp["Xb"]
    nb, q, d = Xb.shape
    got = _device(model, inp, Xb, best)
    floored = model.last_joint_floored.copy()
    assert got.shape == (nb,) and np.all(np.isfinite(got)) and np.all(got >= 0)
    err = np.abs(got - ref["alpha"])
    print("joint %s: max alpha %.3g, share > 0 %.2f, max abs err %.3g, max rel err %.3g, scale %.3g, cond %.3g"
          % (J.case_id(case), ref["alpha"].max(), np.mean(ref["alpha"] > 0), err.max(),
             np.max(err / np.maximum(np.abs(ref["alpha"]), 1e-300) * (ref["alpha"] > 0)), ref["scale"], ref["cond"]))
    np.testing.assert_allclose(got, ref["alpha"], rtol=1e-5, atol=1e-12 * ref["scale"])
    np.testing.assert_array_equal(floored, ref["floored"])
    # a second identical call is bit-identical; the three input layouts are one
    np.testing.assert_array_equal(_device(model, inp, Xb.reshape(nb, q * d), best), got)
    np.testing.assert_array_equal(_device(model, inp, Xb.reshape(nb * q, d), best), got)
    # the values stay on the device for the selection, which ranks batches
    k = min(3, nb)
    idx, val = model.select_topk(k)
    np.testing.assert_array_equal(val, np.sort(got)[::-1][:k])
    # the gradient form: the same value bits, the gradient against the restatement where no sample sits on a kink
    got2, dgot = _device(model, inp, Xb, best, grad=True)
    assert dgot.shape == (nb, q, d) and np.all(np.isfinite(dgot))
    np.testing.assert_array_equal(got2, got)
    keep = ref["margin"] > 1e-6 * ref["scale"]
    gscale = np.abs(ref["dalpha"]).max()
    print("   gradient: %d of %d batches near a kink, max abs err %.3g, gradient scale %.3g"
          % (np.sum(~keep), nb, np.abs(dgot[keep] - ref["dalpha"][keep]).max(), gscale))
    assert gscale > 0
    np.testing.assert_allclose(dgot[keep], ref["dalpha"][keep], rtol=1e-5, atol=1e-12 * gscale)
    again = _device(model, inp, Xb, best, grad=True)
    np.testing.assert_array_equal(again[0], got)
    np.testing.assert_array_equal(again[1], dgot)


@pytest.mark.parametrize("case", J.CHUNK_CASES, ids=[J.case_id(c) for c in J.CHUNK_CASES])
def test_values_across_the_chunk_boundary(case):
    """126, 129 and 136 points: under workspace_mb = 1 (N = 130 padded to 256, m = 2: V of 256 points would fit, V and Sigma of 256 do
    not) the chunks are 128 points -- 42 batches of q = 3 in 126, 16 of q = 8 in 128 -- so the last batches fall into a second chunk; a
    chunk never splits a batch.  The chunked values equal the one-chunk values bit for bit."""
    inp, model, ref, best = _case(case, grad=False)
    whole = _device(model, inp, inp["Xb"], best)
    np.testing.assert_allclose(whole, ref["alpha"], rtol=1e-5, atol=1e-12 * ref["scale"])
    np.testing.assert_array_equal(model.last_joint_floored, ref["floored"])
    model.set_option("workspace_mb", 1)
    try:
        chunked = _device(model, inp, inp["Xb"], best)
    finally:
        model.set_option("workspace_mb", 24576)
    np.testing.assert_array_equal(chunked, whole)
    if inp["Xb"].shape[0] * inp["q"] > 128:                               # 129 and 136 points: past the gradient form's one chunk
        with pytest.raises(ValueError, match="at most 128 points"):
            _device(model, inp, inp["Xb"], best, grad=True)


def _tiny_variance_problem(q=3):
    """A posterior whose latent variance is far below the pivot floor: kernel variance 1e-11 against a noise of 1e-4."""
    kinds = ["se", "matern52"]
    X, Y, var, ls, nz, _ = K.problem(kinds, 12, 3, 1, 11, noise=1e-4)
    var = np.full(2, 1e-11)
    la = K.LookAhead.fit(kinds, X, Y, var, ls, nz)
    model = _fixed_model(kinds, X, Y, var, ls, nz)
    rng = np.random.RandomState(0)
    Z, thetas = rng.normal(size=(64, 2, q)), rng.uniform(-0.5, 0.5, size=(2, 2))
    return la, model, X, Z, thetas


def test_floored_pivots_are_counted_and_harmless():
    """Batches of training inputs under a kernel variance of 1e-11: every pivot is below 1e-10 and floored, on both sides (the pivots
    are ~1e-11 against the floor of 1e-10: no rounding can move one across).  The samples are mu + 1e-5 z."""
    q = 3
    la, model, X, Z, thetas = _tiny_variance_problem(q)
    Xb = X[:2 * q].reshape(2, q, 3)
    best = J.median_best([la], Xb[0], Z, thetas, "neg_sq_dist")[0]
    ref = J.joint(la, Xb, Z, thetas, None, "neg_sq_dist", best=best)
    assert list(ref["floored"]) == [2 * q, 2 * q] and ref["alpha"].max() > 0
    got, dgot = model.acq_joint(Xb, q, _ffi.UTIL_NEG_SQ_DIST, None, thetas, None, Z, best=best, grad=True)
    np.testing.assert_array_equal(model.last_joint_floored, ref["floored"])
    np.testing.assert_allclose(got, ref["alpha"], rtol=1e-5, atol=1e-12 * ref["scale"])
    assert np.all(np.isfinite(dgot))
    np.testing.assert_array_equal(model.acq_joint(Xb, q, _ffi.UTIL_NEG_SQ_DIST, None, thetas, None, Z, best=best), got)


def test_a_duplicate_point_floors_nothing():
    """Two identical points: with a = the point's variance the duplicate's pivot is ((a + tau)^2 - a^2) / (a + tau) ~ 2 tau = 2e-8 mean
    diag Sigma.  The floor is absolute (1e-10), so the pivot is above it where the batch's mean latent variance is above 5e-3: a
    problem with four observations (variances of 0.03 .. 1), not a densely observed one, whose variances of ~1e-4 put even a duplicate
    under the floor.  There the pivot (~1e-9) is also far above the rounding of Sigma's entries (~1e-15): no pivot is floored on either
    side, and the duplicate's sample is the first's plus ~3e-5 z, so the value gate needs no widening."""
    kinds = ["se", "matern52"]
    X, Y, var, ls, nz, _ = K.problem(kinds, 4, 3, 1, 11, noise=1e-4)
    la = K.LookAhead.fit(kinds, X, Y, var, ls, nz)
    rng = np.random.RandomState(3)
    Xb = rng.uniform(size=(4, 3, 3))
    Xb[:, 2] = Xb[:, 0]
    Z, thetas = rng.normal(size=(64, 2, 3)), rng.uniform(-0.5, 0.5, size=(2, 2))
    assert min(np.mean(np.diagonal(la.cov(x, x), axis1=1, axis2=2), 1).min() for x in Xb) > 5e-3
    best = J.median_best([la], Xb[0], Z, thetas, "neg_sq_dist")[0]
    ref = J.joint(la, Xb, Z, thetas, None, "neg_sq_dist", best=best)
    assert ref["floored"].sum() == 0 and ref["alpha"].min() > 0 and ref["cond"] > 1e6
    model = _fixed_model(kinds, X, Y, var, ls, nz)
    got = model.acq_joint(Xb, 3, _ffi.UTIL_NEG_SQ_DIST, None, thetas, None, Z, best=best)
    assert model.last_joint_floored.sum() == 0
    print("duplicate point: cond %.3g, max abs err %.3g, scale %.3g" % (ref["cond"], np.abs(got - ref["alpha"]).max(), ref["scale"]))
    np.testing.assert_allclose(got, ref["alpha"], rtol=1e-5, atol=1e-12 * ref["scale"])


# ---------------------------------------------------------------------------------------------------------------------------------
def test_state_is_left_alone():
    d, N, C = 3, 40, 48
    kinds = PR.MIXED[:3]
    X, Y, var, ls, nz, Xc = K.problem(kinds, N, d, C, 5, noise=1e-4)
    model = _fixed_model(kinds, X, Y, var, ls, nz)
    rng = np.random.RandomState(0)
    support, prob = rng.uniform(-0.5, 0.5, size=(2, 3)), np.array([0.4, 0.6])
    W, A, Zf = rng.normal(size=(25, 3)), rng.uniform(size=(9, d)), rng.normal(size=(4, 3))
    P, Zp = rng.uniform(size=(5, d)), rng.normal(size=(25, 3, 5))
    Z = rng.normal(size=(32, 3, 4))
    nsd = _ffi.UTIL_NEG_SQ_DIST
    model.set_reference_points(A)
    model.set_pending_points(P, Zp, W=W)
    ref_key, pend_key = model._resident.reference, model._resident.pending

    def others():
        return (model.acq_mc(Xc, _ffi.ACQ_EI, nsd, None, support, prob, W=W), model.acq_pending(Xc, nsd, None, support, prob, W=W),
                model.acq_kg(Xc, "closed", nsd, None, support, prob, Zf))
    before = others()
    j1 = model.acq_joint(Xc, 4, nsd, None, support, prob, Z)
    j1g = model.acq_joint(Xc, 4, nsd, None, support, prob, Z, grad=True)
    assert model._resident.reference == ref_key and model._resident.pending == pend_key      # nothing was staged again below
    for u, v in zip(before, others()):
        np.testing.assert_array_equal(u, v)
    np.testing.assert_array_equal(model.acq_joint(Xc, 4, nsd, None, support, prob, Z), j1)
    np.testing.assert_array_equal(j1g[0], j1)
    # an appended observation and a refit: the entry point keeps nothing of its own, the next call answers for the new posterior
    la = None
    for change in ("append", "refit"):
        if change == "append":
            X, Y = np.concatenate([X, Xc[:1]]), [np.concatenate([y, [0.2]]) for y in Y]
        else:
            model.incremental = False
        model.updateModel(X, [y[:, None] for y in Y])
        got = model.acq_joint(Xc, 4, nsd, None, support, prob, Z)
        la = K.LookAhead.fit(kinds, X, Y, var, ls, nz)
        ref = J.joint(la, Xc.reshape(12, 4, d), Z, support, prob, "neg_sq_dist")
        np.testing.assert_allclose(got, ref["alpha"], rtol=1e-5, atol=1e-12 * ref["scale"])
        with pytest.raises(RuntimeError, match="pending points"):
            model.acq_pending(Xc, nsd, None, support, prob, W=W)                             # dropped by the change, as before


def test_every_refusal_names_the_entry_point():
    d, N = 2, 50
    kinds = PR.MIXED[:3]
    X, Y, var, ls, nz, Xc = K.problem(kinds, N, d, 300, 9, noise=1e-4)
    lib, dp = _ffi.load(), _ffi.dptr
    S, q = 4, 2
    Z, th, out = _ffi.f64(np.random.RandomState(1).normal(size=(S, 3, q))), _ffi.f64(np.zeros((2, 3))), np.empty(300 * d)
    Xd = _ffi.f64(Xc[:20])

    def bad(rc, text):
        msg = lib.bocf_last_error()
        assert rc < 0 and b"bocf_acq_joint" in msg and text.encode() in msg, (rc, msg, text)

    def call(h, q=q, z=Z, s=S, util=_ffi.UTIL_NEG_SQ_DIST, params=None, npar=0, theta=th, tdim=3, L=2, best=None, o=out, g=None):
        return lib.bocf_acq_joint(h, q, dp(z), s, util, dp(params), npar, dp(theta), tdim, None, L, dp(best), dp(o), dp(g), None)
    fresh = _ffi.Context(0)
    bad(call(fresh.handle), "not fitted")
    canned = _ffi.Context(0)
    mean, vv, mt = np.zeros((1, 4)), np.ones((1, 4)), np.zeros((1, 3))
    _ffi.check(lib.bocf_set_posterior(canned.handle, 1, 4, 3, dp(mean), dp(vv), dp(mt)), "bocf_set_posterior")
    bad(call(canned.handle, tdim=1), "host-given posterior")
    model = _fixed_model(kinds, X, Y, var, ls, nz)
    model._ensure_fitted()
    h = model._context().handle
    assert lib.bocf_set_candidates(h, dp(Xd), 0) == 0
    bad(call(h), "no resident candidates")
    assert lib.bocf_set_candidates(h, dp(Xd), 20) == 0
    bad(call(h, q=3), "not a multiple of q")
    bad(call(h, q=0), "q out of range")
    bad(call(h, q=9), "q out of range")
    bad(call(h, s=0), "S out of range")
    bad(call(h, s=257), "S out of range")
    bad(call(h, z=None), "null Z")
    bad(call(h, util=_ffi.UTIL_PROGRAM), "BOCF_UTIL_PROGRAM")
    bad(call(h, util=7), "unknown utility kind")
    bad(call(h, L=0), "L out of range")
    bad(call(h, theta=None), "theta")
    bad(call(h, tdim=2), "theta_dim must equal m")
    bad(call(h, util=_ffi.UTIL_ROSENBROCK, tdim=1), "even m")
    bad(call(h, npar=2), "utility parameters")
    bad(call(h, util=_ffi.UTIL_NEG_EXP_COS, tdim=1), "neg_exp_cos needs m weights")
    assert call(h) == 0 and call(h, g=np.empty(20 * d)) == 0
    # the gradient form is one chunk of at most 128 points
    assert lib.bocf_set_candidates(h, dp(_ffi.f64(Xc)), 300) == 0
    assert call(h) == 0
    bad(call(h, g=np.empty(300 * d)), "at most 128 points")
    # more than 16 outputs per hyper-sample
    k17 = ["rbf"] * 17
    X7, Y7, var7, ls7, nz7, _ = K.problem(k17, 12, d, 1, 3, noise=1e-4)
    m17 = _fixed_model(k17, X7, Y7, var7, ls7, nz7)
    m17._ensure_fitted()
    h17 = m17._context().handle
    assert lib.bocf_set_candidates(h17, dp(Xd), 20) == 0
    bad(call(h17, z=_ffi.f64(np.zeros((S, 17, q))), theta=_ffi.f64(np.zeros((2, 16))), tdim=16), "more outputs per hyper-sample")
    # with N = 400 (padded to 512) and 1 MiB not even one chunk of 128 points fits
    X4, Y4, var4, ls4, nz4, _ = K.problem(kinds, 400, d, 1, 10, noise=1e-4)
    bigm = _fixed_model(kinds, X4, Y4, var4, ls4, nz4)
    bigm._ensure_fitted()
    hb = bigm._context().handle
    assert lib.bocf_set_candidates(hb, dp(Xd), 20) == 0
    bigm.set_option("workspace_mb", 1)
    bad(call(hb), "exceeds option workspace_mb")
    bigm.set_option("workspace_mb", 24576)
    assert call(hb) == 0


# ---------------------------------------------------------------------------------------------------------------------------------
def _bo_problem(seed, q):
    np.random.seed(seed)
    d, m = 2, 2
    space = B.Design_space([{'name': 'x', 'type': 'continuous', 'domain': (0, 1), 'dimensionality': d}])
    f = [lambda x: np.sin(3 * x[:, :1]) * x[:, 1:2] + x[:, :1] ** 2, lambda x: np.cos(2 * x[:, 1:2]) + 0.5 * x[:, :1]]
    objective = B.MultiObjective(f, noise_var=[1e-4, 1e-4])
    model = B.multi_outputGP(m, kernel=[B.kern.RBF(d, variance=1.0, lengthscale=0.3, ARD=True) for _ in range(m)], noise_var=[1e-4] * m, fixed_hyps=True)
    U = B.Utility(parameter_dist=B.ParameterDistribution(support=np.array([[0.5, 0.2], [0.1, 0.9]]), prob_dist=np.array([0.5, 0.5])), device="neg_sq_dist")
    opt = B.AcquisitionOptimizer(space, optimizer='lbfgs', n_starting=200, n_anchor=6)
    greedy = B.uEI_pending(model, space, optimizer=opt, utility=U)
    joint = B.uEI_joint(model, space, optimizer=opt, utility=U, q=q, n_samples=64)
    return space, objective, model, greedy, joint, f


def test_uei_joint_through_the_layers():
    q = 3
    space, objective, model, greedy, joint, f = _bo_problem(41, q)
    X0 = np.random.uniform(size=(12, 2))
    model.updateModel(X0, [fj(X0) for fj in f])
    Xr = np.random.uniform(size=(45, q * 2))                               # 45 batches: the gradient form works in groups of 42 and 3
    v, g = joint._compute_acq_withGradients(Xr)
    assert v.shape == (45, 1) and g.shape == (45, q * 2)
    np.testing.assert_array_equal(joint._compute_acq(Xr), v)
    la = K.LookAhead.fit(["rbf", "rbf"], X0, [fj(X0)[:, 0] for fj in f], [1.0, 1.0], [np.full(2, 0.3)] * 2, [1e-4, 1e-4])
    ref = J.joint(la, Xr.reshape(45, q, 2), joint.Z_samples, joint.utility.parameter_dist.support, joint.utility_prob_dist, "neg_sq_dist", grad=True)
    np.testing.assert_allclose(v[:, 0], ref["alpha"], rtol=1e-5, atol=1e-12 * ref["scale"])
    keep = ref["margin"] > 1e-6 * ref["scale"]
    assert np.mean(~keep) <= 1 / 8.0
    np.testing.assert_allclose(g.reshape(45, q, 2)[keep], ref["dalpha"][keep], rtol=1e-5, atol=1e-12 * np.abs(ref["dalpha"]).max())


def test_one_cbo_iteration_with_a_joint_batch():
    q = 3
    space, objective, model, greedy, joint, f = _bo_problem(42, q)
    X0 = np.random.uniform(size=(12, 2))
    ev = B.CompositeJointBatch(joint, q, n_starting=64, n_anchor=8, warm_start=B.CompositeGreedyBatch(greedy, q))
    bo = B.CBO(model, space, objective, joint, ev, X0)
    bo.run_optimization(max_iter=1)
    Xn = bo.X[12:]
    assert bo.X.shape == (12 + q, 2) and Xn.shape == (q, 2) and np.all(Xn >= 0.0) and np.all(Xn <= 1.0)
    info = ev.last_info
    assert info["anchors"].shape == (9, q * 2)                             # eight of the design and the greedy batch
    # the value the evaluator returned is the device's alpha of that batch under the data it was computed for (X0), and no anchor's
    # start beats it, the greedy batch included
    model.updateModel(X0, [y[:12] for y in bo.Y])
    value = joint._compute_acq(Xn.reshape(1, -1))[0, 0]
    starts = joint._compute_acq(info["anchors"])[:, 0]
    scale = max(1.0, np.abs(starts).max())
    print("joint batch alpha %.6g against its anchors' best %.6g (greedy start %.6g)" % (value, starts.max(), starts[-1]))
    np.testing.assert_allclose(starts, info["anchor_values"], rtol=1e-9, atol=1e-12 * scale)          # (the same data fitted again)
    np.testing.assert_allclose(value, info["value"], rtol=1e-9, atol=1e-12 * scale)
    assert value >= starts.max() - 1e-12 * scale
